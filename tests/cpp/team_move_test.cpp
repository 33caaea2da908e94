// team_move_test.cpp -- team_move.h's payload mover on the host, under ASan / UBSan (built host-only
// by tests/test_tcp_build_cpu.py; nothing here runs on a GPU).  Each case runs the 8 lanes of a team
// in a loop -- make_span, move_groups<false> as k_tcp_build calls it or move_groups<true> as
// k_tcp_recv does, the lanes' accumulators added -- over buffers cut so that the sanitizer sees
// every access the kernels' headers rule out:
//   source       a heap block of exactly the segment's 4-B aligned hull [floor4(start), ceil4(end)):
//                a load of a dword that holds no segment byte, on either side, is a heap overflow
//   destination  a heap block that ends at the last stored byte (a store past it is a heap overflow)
//                with guard bytes before the first (a store before it changes them)
// Every stored byte is compared with the source's, and the folded sum with a byte-wise one's
// complement sum written here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "team_move.h"

using namespace vpcsum;

namespace {

constexpr uint32_t kGuard = 32;
uint32_t rng_state = 0x2545f491u;
uint8_t next_byte() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

uint32_t fold(uint64_t x) {
    while (x >> 16) x = (x & 0xffffu) + (x >> 16);
    return (uint32_t)x;
}

long cases = 0, in_one_dword = 0, in_one_group = 0, nothing_stored = 0;

// One segment of `len` bytes whose byte 0 lies at a destination address of residue dres mod 16 and at
// a source address sres mod 4 away from that grid; bytes [store_from, len) are stored.
template <bool SUB>
void run_case(uint32_t len, uint32_t dres, uint32_t sres, uint32_t store_from) {
    const uint32_t stored = len - store_from;
    // source: malloc's block is 16-B aligned, so it is the hull when the segment starts < 4 bytes in
    const uint32_t s_in = (sres + dres) & 3u, hull = (s_in + len + 3u) & ~3u;
    uint8_t* const sbuf = (uint8_t*)malloc(hull);
    for (uint32_t j = 0; j < hull; ++j) sbuf[j] = next_byte();
    const uint8_t* const seg = sbuf + s_in;
    // destination: guard, then the stored bytes up to the block's end
    const uint32_t off = kGuard + ((dres + store_from) & 15u);
    uint8_t* const dbuf = (uint8_t*)malloc(off + stored);
    for (uint32_t j = 0; j < off + stored; ++j) dbuf[j] = (uint8_t)(0xA5u ^ j);
    const uintptr_t v0 = (uintptr_t)dbuf + off - store_from;   // may lie before the block: never dereferenced
    if (((uintptr_t)sbuf & 15u) || ((uintptr_t)dbuf & 15u) || (v0 & 15u) != dres) {
        printf("FAIL: the allocator's blocks are not 16-B aligned\n");
        exit(1);
    }

    const Span sp = make_span(v0, (uintptr_t)seg, len, store_from);
    const uint32_t ng = len ? (sp.hi + 15u) >> 4 : 0u;
    uint64_t total = 0;
    for (uint32_t tl = 0; tl < 8; ++tl) total += move_groups<SUB>(sp, tl, ng);

    // the reference sum: every byte on the destination grid's 16-bit words, low byte at the even address
    uint64_t ref = 0;
    for (uint32_t j = 0; j < len; ++j) ref += ((v0 + j) & 1u) ? (uint32_t)seg[j] << 8 : seg[j];
    bool ok = fold(total) == fold(ref);
    for (uint32_t j = 0; j < off; ++j) ok = ok && dbuf[j] == (uint8_t)(0xA5u ^ j);
    for (uint32_t j = 0; j < stored; ++j) ok = ok && dbuf[off + j] == seg[store_from + j];
    if (!ok) {
        printf("FAIL: %s len %u dres %u sres %u store_from %u: sum %04x want %04x, or a byte differs\n",
               SUB ? "receive" : "build", len, dres, sres, store_from, fold(total), fold(ref));
        exit(1);
    }
    ++cases;
    if (stored == 0) ++nothing_stored;
    if (stored && sp.s_lo / 4u == (sp.s_hi - 1u) / 4u) ++in_one_dword;
    if (stored && sp.s_lo / 16u == (sp.s_hi - 1u) / 16u) ++in_one_group;
    free(dbuf);
    free(sbuf);
}

}  // namespace

int main() {
    for (uint32_t dres = 0; dres < 16; ++dres) {
        for (uint32_t sres = 0; sres < 4; ++sres) {
            for (uint32_t len = 0; len <= 1460; len = len < 80 ? len + 1 : len == 80 ? 1460 : 1461) {
                run_case<false>(len, dres, sres, 0);   // the build: all of it stored, length 0 included
                if (len == 0) continue;
                if (len <= 40) {
                    for (uint32_t from = 0; from <= len; ++from) run_case<true>(len, dres, sres, from);
                } else {
                    const uint32_t froms[] = {0u, 20u, 33u, len - 1u, len};
                    for (uint32_t from : froms) run_case<true>(len, dres, sres, from);
                }
            }
        }
    }
    if (!nothing_stored || !in_one_dword || !in_one_group) {
        printf("FAIL: the cases miss a form of the stored range\n");
        return 1;
    }
    printf("team_move ok: %ld cases, %ld store nothing, %ld store inside one dword, %ld inside one group\n", cases,
           nothing_stored, in_one_dword, in_one_group);
    return 0;
}
