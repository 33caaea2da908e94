// recv_common.h -- what the receive kernels (tcp_recv.hip k_tcp_recv / k_tcp_digest, udp.hip k_udp_recv)
// read besides the segment's own stream, each held once: the descriptor, the pseudo-header's
// addresses and the IPv4 header sum, from the L3 header where it lies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "team_move.h"

namespace vpcsum {

// bytes [p, p + 4) as a little-endian dword, p of any alignment, from the one or two 4-B aligned
// dwords that hold them
__device__ __forceinline__ uint32_t load_shifted(uintptr_t p) {
    const uint32_t sh = (uint32_t)p & 3u;
    const uintptr_t a = p - sh;
    const uint32_t lo = *(gu32_t*)a;
    const uint32_t hi = sh ? *(gu32_t*)(a + 4) : 0u;
    return alignbyte(hi, lo, sh);
}

struct Desc {
    uint64_t l3_off;
    uint32_t l3_len, l4_off, l3_ver, l4_proto, flags;
};
__device__ __forceinline__ Desc load_desc(const vpcsum_desc_t* d) {
    const u32x4a4_t v = *(gu32x4a4_t*)d;   // 16 B at 8-B alignment
    Desc r;
    r.l3_off = ((uint64_t)v.y << 32) | v.x;
    r.l3_len = v.z & 0xffffu;
    r.l4_off = v.z >> 16;
    r.l3_ver = v.w & 0xffu;
    r.l4_proto = (v.w >> 8) & 0xffu;
    r.flags = (v.w >> 16) & 0xffu;
    return r;
}

// Lane tl's share of the pseudo-header's addresses from the L3 header at l3: 2 (IPv4, bytes 12..19)
// or 8 (IPv6, bytes 8..39) dwords, a lane each; they start on an even byte of the header, so their
// sum is in the segment's own 16-bit word order
__device__ __forceinline__ uint32_t recv_addr_sum(uintptr_t l3, uint32_t l3_ver, uint32_t tl) {
    const bool v4 = l3_ver == 4u;
    uint32_t ph = 0;
    if (tl < (v4 ? 2u : 8u)) {
        const uint32_t w = load_shifted(l3 + (v4 ? 12u : 8u) + 4u * tl);
        ph = (w & 0xffffu) + (w >> 16);
    }
    return ph;
}

// The IPv4 header sum of the l4_off header bytes at l3, field masked (an all-zero header gives
// 0xffff): the recomputed sum in bits 0..15, bit 16 set when the stored field equals it.  One lane's
// work; the segment follows the header, so the dword after the header's last is inside the packet.
__device__ __forceinline__ uint32_t recv_ip_header_word(uintptr_t l3, uint32_t l4_off) {
    const uint32_t sh = (uint32_t)l3 & 3u, nw = l4_off >> 2;
    const uintptr_t a = l3 - sh;
    uint64_t ipacc = 0;
    uint32_t cur = *(gu32_t*)a, ip_field = 0;
    for (uint32_t j = 0; j < nw; ++j) {
        // the next dword: always inside the packet (the segment follows the header)
        const uint32_t nxt = (sh || j + 1u < nw) ? *(gu32_t*)(a + 4u * j + 4u) : 0u;
        uint32_t w = alignbyte(nxt, cur, sh);
        cur = nxt;
        if (j == 2u) {
            ip_field = w >> 16;
            w &= 0xffffu;
        }
        ipacc += w;
    }
    const uint32_t ipc = 0xffffu - bswap16(fold64(ipacc));
    return ipc | (bswap16(ip_field) == ipc ? 0x10000u : 0u);
}

}  // namespace vpcsum
