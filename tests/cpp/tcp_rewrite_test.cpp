// tcp_rewrite_test.cpp -- the per-packet TCP rewrite of vproxy_amd/csrc/tcp_rewrite.h (what the
// k_nat_tcp lanes run) and batch_plan.h's nat_tcp_header_end under ASan / UBSan
// (tests/test_tcprw_cpu.py builds and runs it; nothing of the library is linked).  The vectors come
// from a file the test writes; every packet is allocated at its exact size, so a read or write past
// its segment is an error.
//
// File: u32 count, then per vector (little endian): u32 l3_len, u32 l4_off, u8 ver, u8 proto,
// u8 dirty, u8 absent, the 48-byte entry, and three l3_len-byte images: the packet after the
// address / port rewrite with its sums valid, the same after Java's TCP setters (sums left stale),
// and after Java's full recompute of the TCP sum where the setters dirtied it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "batch_plan.h"
#include "tcp_rewrite.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)
#define CHECK_V(cond)                                                                             \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            fprintf(stderr, "%s:%d: vector %u: CHECK(%s) failed\n", __FILE__, __LINE__, i, #cond); \
            if (++g_fail > 20) exit(1);                                                           \
        }                                                                                         \
    } while (0)

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short vectors file\n"); exit(2); }
    return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}
static std::unique_ptr<uint8_t[]> rd(FILE* f, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (fread(p.get(), 1, n, f) != n) { fprintf(stderr, "short vectors file\n"); exit(2); }
    return p;
}

static int run_vectors(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    const uint32_t count = rd32(f);
    uint32_t applied = 0, dirtied = 0, absents = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t len = rd32(f), l4o = rd32(f);
        const auto hdr = rd(f, 4);
        const int proto = hdr[1];
        const bool dirty = hdr[2] != 0, absent = hdr[3] != 0;
        const auto entry = rd(f, 48);
        const auto in = rd(f, len), setters = rd(f, len), full = rd(f, len);
        const TcpRw r = tcp_rw_of_entry(entry.get());
        std::unique_ptr<uint8_t[]> a(new uint8_t[len]);   // exact size
        memcpy(a.get(), in.get(), len);
        if (!r.ops || !tcp_rw_applies(proto, (int)len, (int)l4o)) {
            CHECK_V(!dirty && !absent);
            CHECK_V(memcmp(in.get(), full.get(), len) == 0 && memcmp(in.get(), setters.get(), len) == 0);
            continue;
        }
        ++applied;
        uint8_t* t = a.get() + l4o;
        const uint32_t seg = len - l4o;
        // the strict form: the setters alone, Java's dirty flag, `absent` from the bytes afterwards
        const TcpRes o = tcp_rewrite(t, seg, r);
        CHECK_V(memcmp(a.get(), setters.get(), len) == 0);
        CHECK_V(o.dirty == dirty);
        CHECK_V(o.absent == absent);
        CHECK_V(tcp_mss_absent(t, seg, r) == absent);
        // the RFC 1624 form: the stored sum updated over the changed bytes equals the full recompute
        if (o.dirty) tcp_sum_update(t, o.diff);
        CHECK_V(memcmp(a.get(), full.get(), len) == 0);
        dirtied += dirty;
        absents += absent;
    }
    fclose(f);
    printf("vectors %u applied %u dirty %u absent %u\n", count, applied, dirtied, absents);
    return 0;
}

static vpcsum_desc_t mk(uint16_t len, uint16_t l4_off, uint8_t ver, uint8_t proto) {
    vpcsum_desc_t d;
    memset(&d, 0, sizeof(d));
    d.l3_off = 100;
    d.l3_len = len;
    d.l4_off = l4_off;
    d.l3_ver = ver;
    d.l4_proto = proto;
    return d;
}

static void test_header_extents() {
    CHECK(nat_tcp_header_end(mk(1500, 20, 4, 6)) == 80);     // the longest TCP header a data offset allows
    CHECK(nat_tcp_header_end(mk(50, 20, 4, 6)) == 50);       // never past the packet
    CHECK(nat_tcp_header_end(mk(40, 20, 4, 6)) == 40);       // exactly the 20-byte header
    CHECK(nat_tcp_header_end(mk(39, 20, 4, 6)) == 38);       // a 19-byte segment: as nat_header_end
    CHECK(nat_tcp_header_end(mk(37, 20, 4, 6)) == 20);
    CHECK(nat_tcp_header_end(mk(1500, 60, 4, 6)) == 120);    // IPv4 with IHL 15
    CHECK(nat_tcp_header_end(mk(112, 52, 6, 6)) == 112);     // IPv6 + extension header: through L3 + 111
    CHECK(nat_tcp_header_end(mk(2000, 52, 6, 6)) == 112);
    CHECK(nat_tcp_header_end(mk(2000, 40, 6, 6)) == 100);
    CHECK(nat_tcp_header_end(mk(200, 24, 4, 17)) == 32);     // not TCP: nat_header_end
    CHECK(nat_tcp_header_end(mk(100, 40, 6, 58)) == 44);
    CHECK(nat_tcp_header_end(mk(300, 40, 6, 47)) == 40);
    for (int proto : {1, 6, 17, 47, 58})                      // never below what the first pass can write
        for (int len = 20; len < 140; ++len)
            CHECK(nat_tcp_header_end(mk((uint16_t)len, 20, 4, (uint8_t)proto)) >= nat_header_end(mk((uint16_t)len, 20, 4, (uint8_t)proto)));
}

static void test_decode() {
    uint8_t e[48];
    for (int k = 0; k < 48; ++k) e[k] = (uint8_t)(0xA0 + k);
    e[36] = VPCSUM_NAT_TCP | VPCSUM_NAT_SRC;
    e[38] = 0xff;   // unknown op bits are dropped
    e[39] = 0xd2;   // the flags' two high bits too
    e[40] = 0x05; e[41] = 0x78;
    e[42] = 0xff; e[43] = 0xff; e[44] = 0xff; e[45] = 0xe4;
    TcpRw r = tcp_rw_of_entry(e);
    CHECK(r.ops == 7 && r.flags == 0x12 && r.max_mss == 1400 && r.addend == (uint32_t)-28);
    e[36] = VPCSUM_NAT_SRC;   // without the mask bit: no ops
    CHECK(tcp_rw_of_entry(e).ops == 0);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s vectors-file\n", argv[0]); return 2; }
    test_header_extents();
    test_decode();
    const int rc = run_vectors(argv[1]);
    if (rc) return rc;
    if (g_fail) {
        fprintf(stderr, "tcp_rewrite: %d checks failed\n", g_fail);
        return 1;
    }
    printf("tcp_rewrite ok\n");
    return 0;
}
