// tcp_recv_test.cpp -- the host-checkable rules of the TCP receive (vproxy_amd/csrc/tcp_recv.h: which
// records are refused, hlen, data_len, the stored count) in a stand-alone program under ASan / UBSan
// (tests/test_tcp_recv_cpu.py builds and runs it; nothing of the library is linked).  Every refusal
// of include/vpcsum.h's list at the value that is accepted and at the first that is not, one value
// well inside each refusal, the bounds at UINT64_MAX, and skip == data_len.  The arena is allocated
// at its exact size and byte 12 is read through a checked accessor, so a rule that looked at the
// arena before the descriptor allowed it would be an error here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tcp_recv.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)

static std::vector<uint8_t> g_arena;
static int g_reads = 0;

struct Byte12 {
    uint32_t operator()(uint64_t off) const {
        ++g_reads;
        if (off >= g_arena.size()) {
            fprintf(stderr, "byte 12 read at %llu outside the arena of %zu bytes\n", (unsigned long long)off, g_arena.size());
            exit(1);
        }
        return g_arena[off];
    }
};

static vpcsum_desc_t mk_desc(uint64_t l3_off, uint32_t l3_len, uint32_t l4_off, int ver, int proto = 6, int flags = -1) {
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

static vpcsum_tcprx_t mk_rx(uint64_t dst_off, uint32_t dst_cap, uint32_t skip, int ops = VPCSUM_TCPRX_STORE, int rsv = 0) {
    vpcsum_tcprx_t r;
    memset(&r, 0, sizeof(r));
    r.dst_off = dst_off;
    r.dst_cap = dst_cap;
    r.skip = (uint16_t)skip;
    r.ops = (uint8_t)ops;
    r.rsv = (uint8_t)rsv;
    return r;
}

static bool ok(const vpcsum_desc_t& d, const vpcsum_tcprx_t& r, uint64_t dst_len, TcpRecvPlan* p = nullptr,
               uint64_t arena_len = UINT64_MAX) {
    TcpRecvPlan q;
    const bool v = tcp_recv_plan(d, r, arena_len == UINT64_MAX ? g_arena.size() : arena_len, dst_len, Byte12(), &q);
    if (!v) CHECK(q.hlen == 0 && q.data_len == 0 && q.stored == 0);
    if (p) *p = q;
    return v;
}

int main() {
    // an arena of exactly 200 bytes; an IPv4 packet at 10 (IHL 5, a 32-byte TCP header, 68 payload
    // bytes: l3_len 120) and an IPv6 one at 130 whose segment is the last 22 bytes of the arena
    g_arena.assign(200, 0);
    g_arena[10 + 20 + 12] = 0x80;           // data offset 8
    g_arena[130 + 48 + 12] = 0x50;          // data offset 5 (l4_off 48: 22-byte segment)
    const vpcsum_desc_t v4 = mk_desc(10, 120, 20, 4), v6 = mk_desc(130, 70, 48, 6);
    const vpcsum_tcprx_t r0 = mk_rx(0, 1000, 0);
    TcpRecvPlan p;

    CHECK(ok(v4, r0, 1000, &p) && p.hlen == 32 && p.data_len == 68 && p.stored == 68);
    CHECK(ok(v6, r0, 1000, &p) && p.hlen == 20 && p.data_len == 2 && p.stored == 2);

    // the descriptor's refusals read nothing of the arena
    g_reads = 0;
    CHECK(!ok(mk_desc(10, 120, 20, 4, 17), r0, 1000) && !ok(mk_desc(10, 120, 20, 4, 0), r0, 1000));      // l4_proto
    CHECK(!ok(mk_desc(10, 120, 20, 5), r0, 1000) && !ok(mk_desc(10, 120, 20, 0), r0, 1000));              // l3_ver
    CHECK(!ok(mk_desc(10, 120, 20, 4, 6, VPCSUM_F_IP), r0, 1000) && !ok(mk_desc(10, 120, 20, 4, 6, 0), r0, 1000));   // no F_L4
    CHECK(ok(mk_desc(10, 120, 20, 4, 6, VPCSUM_F_L4), r0, 1000));
    g_reads = 0;
    CHECK(!ok(mk_desc(10, 120, 20, 4, 6, VPCSUM_F_L4 | VPCSUM_F_L4P), r0, 1000));
    CHECK(!ok(mk_desc(10, 120, 20, 4, 6, VPCSUM_F_L4 | VPCSUM_F_RAW), r0, 1000));
    CHECK(!ok(mk_desc(10, 120, 20, 4, 6, VPCSUM_F_L4 | VPCSUM_F_PRE), r0, 1000));
    CHECK(!ok(mk_desc(130, 70, 48, 6, 6, VPCSUM_F_L4 | VPCSUM_F_IP), r0, 1000));                          // F_IP on IPv6
    CHECK(!ok(mk_desc(10, 120, 121, 4), r0, 1000) && !ok(mk_desc(10, 120, 124, 4), r0, 1000));            // l4_off > l3_len
    CHECK(!ok(mk_desc(10, 120, 16, 4), r0, 1000) && !ok(mk_desc(10, 120, 22, 4), r0, 1000));              // compute's l4_off rule
    CHECK(!ok(mk_desc(130, 70, 39, 6), r0, 1000) && !ok(mk_desc(130, 70, 0, 6), r0, 1000));
    CHECK(!ok(mk_desc(131, 70, 48, 6), r0, 1000));                                                        // one byte past the arena
    CHECK(!ok(mk_desc(201, 0, 0, 6), r0, 1000) && !ok(mk_desc(4000, 70, 48, 6), r0, 1000));
    CHECK(!ok(mk_desc(UINT64_MAX, 70, 48, 6), r0, 1000) && !ok(mk_desc(UINT64_MAX - 69, 70, 48, 6), r0, 1000));   // no wrap
    CHECK(!ok(mk_desc(UINT64_MAX - 30, 70, 48, 6), r0, 1000, nullptr, UINT64_MAX - 1));   // ... with an arena that long, too
    CHECK(!ok(mk_desc(130, 67, 48, 6), r0, 1000) && !ok(mk_desc(130, 48, 48, 6), r0, 1000));              // segment of 19 and of 0 bytes
    CHECK(!ok(mk_desc(10, 39, 20, 4), r0, 1000));
    CHECK(!ok(v4, mk_rx(0, 1000, 0, 2), 1000) && !ok(v4, mk_rx(0, 1000, 0, 0x81), 1000) && !ok(v4, mk_rx(0, 1000, 0, 1, 1), 1000) &&
          !ok(v4, mk_rx(0, 1000, 0, 0, 0xff), 1000));                                                     // ops, rsv
    CHECK(g_reads == 0);
    CHECK(ok(mk_desc(130, 68, 48, 6), r0, 1000, &p) && p.data_len == 0 && p.stored == 0);                 // a 20-byte segment
    CHECK(ok(mk_desc(UINT64_MAX - 100, 70, 48, 6), mk_rx(0, 0, 0, 0), 0, nullptr, 0) == false);

    // the data offset: below 5, and past the segment
    for (int doff = 0; doff < 16; ++doff) {
        g_arena[130 + 48 + 12] = (uint8_t)((doff << 4) | 0x0f);   // the low nibble is not the offset
        const bool want = doff == 5;                              // 22-byte segment: 24 is too long
        CHECK(ok(v6, r0, 1000, &p) == want);
        g_arena[10 + 20 + 12] = (uint8_t)(doff << 4);
        CHECK(ok(v4, r0, 1000, &p) == (doff >= 5) && (doff < 5 || (p.hlen == 4u * doff && p.data_len == 100u - 4u * doff)));
    }
    g_arena[10 + 20 + 12] = 0xf0;
    CHECK(ok(mk_desc(10, 80, 20, 4), r0, 1000, &p) && p.hlen == 60 && p.data_len == 0);                   // hlen == the segment
    CHECK(!ok(mk_desc(10, 79, 20, 4), r0, 1000) && !ok(mk_desc(10, 41, 20, 4), r0, 1000));                // hlen one past it; far past
    g_arena[10 + 20 + 12] = 0x80;
    g_arena[130 + 48 + 12] = 0x50;

    // skip: up to data_len, which stores nothing
    CHECK(ok(v4, mk_rx(5, 1000, 67), 1000, &p) && p.stored == 1);
    CHECK(ok(v4, mk_rx(5, 0, 68), 1000, &p) && p.stored == 0 && p.data_len == 68);   // skip == data_len, no room needed
    CHECK(ok(v4, mk_rx(1000, 0, 68), 1000, &p) && p.stored == 0);                     // ... at the destination's very end
    CHECK(!ok(v4, mk_rx(5, 1000, 69), 1000) && !ok(v4, mk_rx(5, 1000, 65535), 1000));
    CHECK(!ok(v4, mk_rx(5, 1000, 69, 0), 1000));                                      // verify only: skip still checked
    // verify only: no room, no destination
    CHECK(ok(v4, mk_rx(UINT64_MAX, 0, 0, 0), 0, &p) && p.stored == 0 && p.data_len == 68);
    // dst_cap exact and one short
    CHECK(ok(v4, mk_rx(0, 68, 0), 1000) && !ok(v4, mk_rx(0, 67, 0), 1000) && !ok(v4, mk_rx(0, 0, 0), 1000));
    CHECK(ok(v4, mk_rx(0, 58, 10), 1000, &p) && p.stored == 58 && !ok(v4, mk_rx(0, 57, 10), 1000));
    // dst_off + stored against dst_len, without wrapping
    CHECK(ok(v4, mk_rx(932, 68, 0), 1000) && !ok(v4, mk_rx(933, 68, 0), 1000) && !ok(v4, mk_rx(1001, 68, 0), 1000) &&
          !ok(v4, mk_rx(5000, 68, 0), 1000));
    CHECK(!ok(v4, mk_rx(UINT64_MAX, 68, 0), 1000) && !ok(v4, mk_rx(UINT64_MAX - 67, 68, 0), 1000) &&
          !ok(v4, mk_rx(UINT64_MAX - 10, 68, 0), UINT64_MAX));
    CHECK(ok(v4, mk_rx(UINT64_MAX - 68, 68, 0), UINT64_MAX) && !ok(v4, mk_rx(UINT64_MAX - 67, 68, 0), UINT64_MAX));
    CHECK(ok(v4, mk_rx(1001, 0, 68), 1000) == false);   // an empty store past the destination is still outside it

    static_assert(sizeof(vpcsum_tcprx_t) == 16 && alignof(vpcsum_tcprx_t) == 8, "record layout");
    static_assert(sizeof(vpcsum_tcpinfo_t) == 16 && alignof(vpcsum_tcpinfo_t) == 4, "digest layout");
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("tcp_recv ok\n");
    return 0;
}
