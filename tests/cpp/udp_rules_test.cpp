// udp_rules_test.cpp -- the host-checkable rules of the UDP datagram build and receive
// (vproxy_amd/csrc/udp_build.h, udp_recv.h) in a stand-alone program under ASan / UBSan
// (tests/test_udp_cpu.py builds and runs it; nothing of the library is linked).  The header words
// against a byte-wise restatement of the field list of include/vpcsum.h with byte-wise RFC 1071 sums,
// the 0 -> 0xffff rule, every refusal at the value that is accepted and at the first that is not
// (data_len near 2^32 and offsets near 2^64 included), the receive's refusals and verdicts.  With a
// frame's hex on the command line (kat.json udpIpv4Example) its 42 header bytes are rebuilt too.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "udp_build.h"
#include "udp_recv.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)

// RFC 1071 over bytes, big-endian words, end-around carry, complemented
static uint32_t csum_bytes(const std::vector<uint8_t>& b) {
    uint64_t s = 0;
    for (size_t i = 0; i < b.size(); i += 2) s += ((uint32_t)b[i] << 8) | (i + 1 < b.size() ? b[i + 1] : 0u);
    while (s >> 16) s = (s & 0xffff) + (s >> 16);
    return (uint32_t)(~s & 0xffff);
}

static vpcsum_udphdr_t mk_hdr(int ver, int l2) {
    vpcsum_udphdr_t h;
    memset(&h, 0, sizeof(h));
    for (int i = 0; i < 6; ++i) h.eth_dst[i] = (uint8_t)(0xa0 + i), h.eth_src[i] = (uint8_t)(0xb0 + i);
    h.l2_len = (uint8_t)l2;
    h.l3_ver = (uint8_t)ver;
    h.tos = 0xb8;
    h.ttl = 63;
    for (int i = 0; i < 16; ++i) h.src[i] = (uint8_t)(0x11 + i), h.dst[i] = (uint8_t)(0x91 + 3 * i);
    h.sport[0] = 0x00; h.sport[1] = 0x35;
    h.dport[0] = 0xc9; h.dport[1] = 0x14;
    h.ident[0] = 0x37; h.ident[1] = 0xbd;
    h.frag[0] = 0x40; h.frag[1] = 0x00;
    return h;
}

// the frame's header bytes and sums from the field list, byte by byte
static std::vector<uint8_t> want_header(const vpcsum_udphdr_t& h, const std::vector<uint8_t>& pay, uint32_t* ipc, uint32_t* l4c) {
    const uint32_t d = (uint32_t)pay.size();
    std::vector<uint8_t> eth, ip, udp, ph;
    const bool v4 = h.l3_ver == 4;
    if (h.l2_len == 14) {
        eth.insert(eth.end(), h.eth_dst, h.eth_dst + 6);
        eth.insert(eth.end(), h.eth_src, h.eth_src + 6);
        eth.push_back(v4 ? 0x08 : 0x86);
        eth.push_back(v4 ? 0x00 : 0xdd);
    }
    if (v4) {
        const uint32_t tl = 28 + d;
        ip = {0x45, h.tos, (uint8_t)(tl >> 8), (uint8_t)tl, h.ident[0], h.ident[1], h.frag[0], h.frag[1], h.ttl, 0x11, 0, 0};
        ip.insert(ip.end(), h.src, h.src + 4);
        ip.insert(ip.end(), h.dst, h.dst + 4);
        *ipc = csum_bytes(ip);
        ip[10] = (uint8_t)(*ipc >> 8);
        ip[11] = (uint8_t)*ipc;
        ph.insert(ph.end(), h.src, h.src + 4);
        ph.insert(ph.end(), h.dst, h.dst + 4);
        ph.push_back(0); ph.push_back(17);
        ph.push_back((uint8_t)((8 + d) >> 8)); ph.push_back((uint8_t)(8 + d));
    } else {
        const uint32_t pl = 8 + d;
        ip = {(uint8_t)(0x60 | (h.tos >> 4)), (uint8_t)(h.tos << 4), 0, 0, (uint8_t)(pl >> 8), (uint8_t)pl, 0x11, h.ttl};
        ip.insert(ip.end(), h.src, h.src + 16);
        ip.insert(ip.end(), h.dst, h.dst + 16);
        *ipc = 0;
        ph.insert(ph.end(), h.src, h.src + 16);
        ph.insert(ph.end(), h.dst, h.dst + 16);
        ph.push_back((uint8_t)(pl >> 24)); ph.push_back((uint8_t)(pl >> 16)); ph.push_back((uint8_t)(pl >> 8)); ph.push_back((uint8_t)pl);
        ph.push_back(0); ph.push_back(0); ph.push_back(0); ph.push_back(17);
    }
    udp = {h.sport[0], h.sport[1], h.dport[0], h.dport[1], (uint8_t)((8 + d) >> 8), (uint8_t)(8 + d), 0, 0};
    std::vector<uint8_t> all = ph;
    all.insert(all.end(), udp.begin(), udp.end());
    all.insert(all.end(), pay.begin(), pay.end());
    uint32_t c = csum_bytes(all);
    if (c == 0) c = 0xffff;
    *l4c = c;
    udp[6] = (uint8_t)(c >> 8);
    udp[7] = (uint8_t)c;
    std::vector<uint8_t> out = eth;
    out.insert(out.end(), ip.begin(), ip.end());
    out.insert(out.end(), udp.begin(), udp.end());
    return out;
}

// the same through udp_build.h, the payload summed as little-endian dwords from its first byte (an even
// offset of the segment: no swap)
static std::vector<uint8_t> got_header(const vpcsum_udphdr_t& h, const std::vector<uint8_t>& pay, uint32_t* ipc, uint32_t* l4c) {
    uint32_t t[16];
    tcp_build_template_words(h, t);
    CHECK(udp_build_hdr_ok(t));
    const uint32_t d = (uint32_t)pay.size();
    uint64_t acc = 0;
    for (uint32_t i = 0; i < d; ++i) acc += (uint64_t)pay[i] << (8 * (i & 3));
    UdpBuildWords w;
    udp_build_words(t, d, w);
    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t ip_field = v4 ? 0xffffu - tb_fold64(udp_build_ip_header_sum(w)) : 0u;
    const uint32_t l4_field = udp_build_l4_field(tb_fold64(udp_build_l4_header_sum(t, w, d) + tb_fold64(acc)));
    udp_build_set_sums(w, v4, ip_field, l4_field);
    *ipc = tb_bswap16(ip_field);
    *l4c = tb_bswap16(l4_field);
    uint8_t buf[kUdpBuildMaxHeader];
    const uint32_t n = udp_build_header_bytes(w, t, buf);
    CHECK(n == udp_build_header_len(t) && n <= kUdpBuildMaxHeader);
    return std::vector<uint8_t>(buf, buf + n);
}

static bool fits(const vpcsum_udphdr_t& h, uint64_t frame_off, uint64_t data_off, uint32_t cap, uint32_t d, uint64_t dst_len,
                 uint64_t src_len) {
    uint32_t t[16];
    tcp_build_template_words(h, t);
    return udp_build_hdr_ok(t) && udp_build_fits(t, frame_off, data_off, cap, d, dst_len, src_len);
}

static vpcsum_desc_t mk_desc(uint64_t l3_off, uint32_t l3_len, uint32_t l4_off, int ver, int proto = 17, int flags = -1) {
    vpcsum_desc_t d;
    memset(&d, 0, sizeof(d));
    d.l3_off = l3_off;
    d.l3_len = (uint16_t)l3_len;
    d.l4_off = (uint16_t)l4_off;
    d.l3_ver = (uint8_t)ver;
    d.l4_proto = (uint8_t)proto;
    d.flags = (uint8_t)(flags >= 0 ? flags : (VPCSUM_F_L4 | (ver == 4 ? VPCSUM_F_IP : 0)));
    return d;
}

static vpcsum_udprx_t mk_rx(uint64_t dst_off, uint32_t dst_cap, int ops = VPCSUM_UDPRX_STORE, int rsv_at = -1) {
    vpcsum_udprx_t r;
    memset(&r, 0, sizeof(r));
    r.dst_off = dst_off;
    r.dst_cap = dst_cap;
    r.ops = (uint8_t)ops;
    if (rsv_at >= 0) r.rsv[rsv_at] = 1;
    return r;
}

static bool rok(const vpcsum_desc_t& d, const vpcsum_udprx_t& r, uint64_t dst_len, uint32_t* stored = nullptr,
                uint64_t arena_len = 200) {
    uint32_t st = 77;
    const bool v = udp_recv_plan(d, r, arena_len, dst_len, &st);
    if (!v) CHECK(st == 0);
    if (stored) *stored = st;
    return v;
}

int main(int argc, char** argv) {
    // ---- build: header bytes and sums, IPv4 / IPv6 x l2_len 0 / 14, several payloads
    for (int ver : {4, 6})
        for (int l2 : {0, 14})
            for (uint32_t d : {0u, 1u, 2u, 3u, 7u, 61u, 1472u}) {
                std::vector<uint8_t> pay(d);
                for (uint32_t i = 0; i < d; ++i) pay[i] = (uint8_t)(i * 37 + 11);
                const vpcsum_udphdr_t h = mk_hdr(ver, l2);
                uint32_t wi, wl, gi, gl;
                const std::vector<uint8_t> want = want_header(h, pay, &wi, &wl), got = got_header(h, pay, &gi, &gl);
                CHECK(want == got && wi == gi && wl == gl);
                CHECK(got.size() == (size_t)l2 + (ver == 4 ? 20 : 40) + 8);
            }
    // ---- a sum that computes to 0 is stored as 0xffff: one aligned payload word takes the sum the
    // datagram has with that word 0
    for (int ver : {4, 6}) {
        std::vector<uint8_t> pay(64);
        for (uint32_t i = 0; i < 64; ++i) pay[i] = (uint8_t)(i * 5 + 3);
        pay[2] = pay[3] = 0;
        const vpcsum_udphdr_t h = mk_hdr(ver, 14);
        uint32_t wi, wl, gi, gl;
        want_header(h, pay, &wi, &wl);
        pay[2] = (uint8_t)(wl >> 8);
        pay[3] = (uint8_t)wl;
        const std::vector<uint8_t> want = want_header(h, pay, &wi, &wl), got = got_header(h, pay, &gi, &gl);
        CHECK(wl == 0xffff && gl == 0xffff && want == got);
    }
    CHECK(udp_build_l4_field(0xffffu) == 0xffffu && udp_build_l4_field(0xfffeu) == 1u && udp_build_l4_field(1u) == 0xfffeu);

    // ---- build: refusals
    {
        uint32_t t[16];
        vpcsum_udphdr_t h = mk_hdr(4, 14);
        CHECK(udp_build_dg_ok(0, 1, 0) && !udp_build_dg_ok(1, 1, 0) && !udp_build_dg_ok(0, 0, 0) && !udp_build_dg_ok(0, 1, 1) &&
              !udp_build_dg_ok(0, 1, 0x80000000u) && !udp_build_dg_ok(UINT32_MAX, UINT32_MAX, 0));
        for (int at = 52; at < 64; ++at) {   // ack, window and rsv must be 0; ident and frag are taken
            vpcsum_udphdr_t g = h;
            ((uint8_t*)&g)[at] ^= 0x10;
            tcp_build_template_words(g, t);
            CHECK(udp_build_hdr_ok(t) == (at >= 58 && at < 62));
        }
        for (int ver = 0; ver < 8; ++ver)
            for (int l2 : {0, 1, 13, 14, 15, 18}) {
                const vpcsum_udphdr_t g = mk_hdr(ver, l2);
                tcp_build_template_words(g, t);
                CHECK(udp_build_hdr_ok(t) == ((ver == 4 || ver == 6) && (l2 == 0 || l2 == 14)));
            }
        const vpcsum_udphdr_t h6 = mk_hdr(6, 0);
        const uint64_t big = 1ull << 40;
        // the length fields: IPv4 28 + d, IPv6 8 + d, at 65535 and one past; far past; near 2^32
        CHECK(fits(h, 0, 0, 70000, 65507, big, big) && !fits(h, 0, 0, 70000, 65508, big, big));
        CHECK(fits(h6, 0, 0, 70000, 65527, big, big) && !fits(h6, 0, 0, 70000, 65528, big, big));
        for (uint32_t d : {65536u, 0x7fffffffu, 0x80000000u, 0xffffffe3u, 0xffffffe4u, 0xfffffff7u, 0xfffffff8u, 0xffffffffu})
            CHECK(!fits(h, 0, 0, UINT32_MAX, d, UINT64_MAX, UINT64_MAX) && !fits(h6, 0, 0, UINT32_MAX, d, UINT64_MAX, UINT64_MAX));
        // frame_cap: L exact and one short
        CHECK(fits(h, 0, 0, 42 + 100, 100, big, big) && !fits(h, 0, 0, 42 + 99, 100, big, big) && !fits(h, 0, 0, 0, 0, big, big));
        CHECK(fits(h6, 0, 0, 48, 0, big, big) && !fits(h6, 0, 0, 47, 0, big, big));
        // the arenas, without wrapping
        CHECK(fits(h, 858, 0, 200, 100, 1000, 100) && !fits(h, 859, 0, 200, 100, 1000, 100) && !fits(h, 1001, 0, 200, 100, 1000, 100));
        CHECK(fits(h, 0, 900, 200, 100, 1000, 1000) && !fits(h, 0, 901, 200, 100, 1000, 1000) && !fits(h, 0, 1001, 200, 0, 1000, 1000));
        CHECK(fits(h, 0, 1000, 200, 0, 1000, 1000));   // an empty payload at the source's end
        CHECK(!fits(h, UINT64_MAX, 0, 200, 100, 1000, 1000) && !fits(h, UINT64_MAX - 141, 0, 200, 100, UINT64_MAX, 1000) &&
              fits(h, UINT64_MAX - 142, 0, 200, 100, UINT64_MAX, 1000));
        CHECK(!fits(h, 0, UINT64_MAX, 200, 100, 1000, 1000) && !fits(h, 0, UINT64_MAX - 99, 200, 100, 1000, UINT64_MAX) &&
              fits(h, 0, UINT64_MAX - 100, 200, 100, 1000, UINT64_MAX));
        CHECK(fits(h, 0, 0, 42, 0, 42, 0) && !fits(h, 0, 0, 42, 0, 41, 0));   // data_len 0 is a legal datagram
    }

    // ---- the staged span and the rebase, on UDP records (tcp_build.h's helpers)
    {
        vpcsum_udpdg_t r[4];
        memset(r, 0, sizeof(r));
        r[0].data_off = 100; r[0].data_len = 50;
        r[1].data_off = 40;  r[1].data_len = 0;           // empty: not in the span
        r[2].data_off = 990; r[2].data_len = 20;          // leaves the source: not in the span
        r[3].data_off = 300; r[3].data_len = 0x10000;     // a 32-bit length, outside too
        TcpPayloadSpan sp;
        CHECK(tcp_build_payload_span(r, 4, 1000, 64, &sp) && sp.lo == 100 && sp.len == 50);
        CHECK(!tcp_build_payload_span(r, 4, 1000, 49, &sp));
        tcp_build_rebase_payloads(r, 4, 1000, sp.lo);
        CHECK(r[0].data_off == 0 && r[1].data_off == 0 && r[2].data_off == UINT64_MAX && r[3].data_off == UINT64_MAX);
    }

    // ---- receive: refusals.  An arena of 200 bytes: IPv4 at 10 (l3_len 120, l4_off 20: a segment of
    // 100), IPv6 at 130 whose segment is the last 8 bytes of the arena
    {
        const vpcsum_desc_t v4 = mk_desc(10, 120, 20, 4), v6 = mk_desc(130, 70, 62, 6);
        const vpcsum_udprx_t r0 = mk_rx(0, 1000);
        uint32_t st;
        CHECK(rok(v4, r0, 1000, &st) && st == 92);
        CHECK(rok(v6, r0, 1000, &st) && st == 0);                                                        // seg_len exactly 8
        CHECK(rok(v6, mk_rx(1000, 0), 1000, &st) && st == 0 && !rok(v6, mk_rx(1001, 0), 1000));
        CHECK(!rok(mk_desc(10, 120, 20, 4, 6), r0, 1000) && !rok(mk_desc(10, 120, 20, 4, 0), r0, 1000));   // l4_proto
        CHECK(!rok(mk_desc(10, 120, 20, 5), r0, 1000) && !rok(mk_desc(10, 120, 20, 0), r0, 1000));         // l3_ver
        CHECK(!rok(mk_desc(10, 120, 20, 4, 17, VPCSUM_F_IP), r0, 1000) && !rok(mk_desc(10, 120, 20, 4, 17, 0), r0, 1000));
        CHECK(rok(mk_desc(10, 120, 20, 4, 17, VPCSUM_F_L4), r0, 1000));
        CHECK(!rok(mk_desc(10, 120, 20, 4, 17, VPCSUM_F_L4 | VPCSUM_F_L4P), r0, 1000));
        CHECK(!rok(mk_desc(10, 120, 20, 4, 17, VPCSUM_F_L4 | VPCSUM_F_RAW), r0, 1000));
        CHECK(!rok(mk_desc(10, 120, 20, 4, 17, VPCSUM_F_L4 | VPCSUM_F_PRE), r0, 1000));
        CHECK(!rok(mk_desc(130, 70, 62, 6, 17, VPCSUM_F_L4 | VPCSUM_F_IP), r0, 1000));                     // F_IP on IPv6
        CHECK(!rok(mk_desc(10, 120, 121, 4), r0, 1000) && !rok(mk_desc(10, 120, 124, 4), r0, 1000));       // l4_off > l3_len
        CHECK(!rok(mk_desc(10, 120, 16, 4), r0, 1000) && !rok(mk_desc(10, 120, 22, 4), r0, 1000));         // compute's l4_off rule
        CHECK(!rok(mk_desc(130, 70, 39, 6), r0, 1000) && !rok(mk_desc(130, 70, 0, 6), r0, 1000));
        CHECK(!rok(mk_desc(131, 70, 62, 6), r0, 1000) && !rok(mk_desc(4000, 70, 62, 6), r0, 1000));        // past the arena
        CHECK(!rok(mk_desc(UINT64_MAX, 70, 62, 6), r0, 1000) && !rok(mk_desc(UINT64_MAX - 69, 70, 62, 6), r0, 1000));   // no wrap
        CHECK(!rok(mk_desc(UINT64_MAX - 30, 70, 62, 6), r0, 1000, nullptr, UINT64_MAX - 1));
        CHECK(!rok(mk_desc(130, 69, 62, 6), r0, 1000) && !rok(mk_desc(130, 62, 62, 6), r0, 1000));         // segments of 7 and 0 bytes
        CHECK(!rok(mk_desc(10, 27, 20, 4), r0, 1000) && rok(mk_desc(10, 28, 20, 4), r0, 1000, &st) && st == 0);
        CHECK(!rok(v4, mk_rx(0, 1000, 2), 1000) && !rok(v4, mk_rx(0, 1000, 0x81), 1000));                  // ops
        CHECK(!rok(v4, mk_rx(0, 1000, 1, 0), 1000) && !rok(v4, mk_rx(0, 1000, 1, 1), 1000) && !rok(v4, mk_rx(0, 1000, 0, 2), 1000));   // rsv
        // verify only: no room, no destination
        CHECK(rok(v4, mk_rx(UINT64_MAX, 0, 0), 0, &st) && st == 0);
        // dst_cap exact and one short; dst_off + stored against dst_len, without wrapping
        CHECK(rok(v4, mk_rx(0, 92), 1000) && !rok(v4, mk_rx(0, 91), 1000) && !rok(v4, mk_rx(0, 0), 1000));
        CHECK(rok(v4, mk_rx(908, 92), 1000) && !rok(v4, mk_rx(909, 92), 1000) && !rok(v4, mk_rx(5000, 92), 1000));
        CHECK(!rok(v4, mk_rx(UINT64_MAX, 92), 1000) && !rok(v4, mk_rx(UINT64_MAX - 91, 92), 1000) &&
              !rok(v4, mk_rx(UINT64_MAX - 91, 92), UINT64_MAX) && rok(v4, mk_rx(UINT64_MAX - 92, 92), UINT64_MAX));
    }
    // ---- receive: the verdict (host-order values)
    CHECK(udp_recv_l4c(0) == 0xffff && udp_recv_l4c(0x1234) == 0x1234 && udp_recv_l4c(0xffff) == 0xffff);
    CHECK(udp_recv_l4_status(0x1234, 0x1234) == VPCSUM_S_L4_OK && udp_recv_l4_status(0x1235, 0x1234) == 0);
    CHECK(udp_recv_l4_status(0xffff, 0) == VPCSUM_S_L4_OK);                   // a stored 0xffff on a sum of 0
    CHECK(udp_recv_l4_status(0, 0) == VPCSUM_S_UDP_NOCSUM);                   // a stored 0: no checksum, never OK
    CHECK(udp_recv_l4_status(0, 0x1234) == VPCSUM_S_UDP_NOCSUM && udp_recv_l4_status(0, 0xffff) == VPCSUM_S_UDP_NOCSUM);

    static_assert(sizeof(vpcsum_udpdg_t) == 32 && alignof(vpcsum_udpdg_t) == 8, "record layout");
    static_assert(sizeof(vpcsum_udprx_t) == 16 && alignof(vpcsum_udprx_t) == 8, "record layout");

    // ---- the reference frame (Ethernet / IPv4 / UDP): its 42 header bytes rebuilt from its own fields
    bool with_ref = false;
    if (argc > 1) {
        const std::string hex = argv[1];
        std::vector<uint8_t> raw(hex.size() / 2);
        for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        CHECK(raw.size() > 42 && raw[12] == 0x08 && raw[13] == 0x00 && raw[14] == 0x45 && raw[23] == 17);
        vpcsum_udphdr_t h;
        memset(&h, 0, sizeof(h));
        memcpy(h.eth_dst, &raw[0], 6);
        memcpy(h.eth_src, &raw[6], 6);
        h.l2_len = 14;
        h.l3_ver = 4;
        h.tos = raw[15];
        h.ttl = raw[22];
        memcpy(h.ident, &raw[18], 2);
        memcpy(h.frag, &raw[20], 2);
        memcpy(h.src, &raw[26], 4);
        memcpy(h.dst, &raw[30], 4);
        memcpy(h.sport, &raw[34], 2);
        memcpy(h.dport, &raw[36], 2);
        const uint32_t total = ((uint32_t)raw[16] << 8) | raw[17];
        const std::vector<uint8_t> pay(raw.begin() + 42, raw.begin() + 14 + total);
        uint32_t gi, gl;
        const std::vector<uint8_t> got = got_header(h, pay, &gi, &gl);
        CHECK(got.size() == 42 && memcmp(got.data(), raw.data(), 42) == 0);
        printf("reference header %zu bytes, %zu payload bytes, ip sum %04x, udp sum %04x\n", got.size(), pay.size(), gi, gl);
        with_ref = true;
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("udp_rules ok%s\n", with_ref ? " (with the reference frame)" : "");
    return 0;
}
