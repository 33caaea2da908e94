// tcp_recv.hip -- k_tcp_recv (vpcsum_tcp_recv_async) and k_tcp_digest (vpcsum_tcp_digest_async): the
// receive side of the userspace TCP stack, tcp_build.hip run the other way.  Per record the segment is
// read once; every byte is added to the TCP sum and, when it is payload past the record's `skip`,
// stored into the receive buffer from the register that summed it.  No second pass over the payload.
//
// Segment: a team of 8 lanes per record runs team_move.h's mover over it (the grid, the source
// loads, the edges and the sum are described there).  The whole segment is laid on the destination's
// grid through a virtual destination address V0 = dst + dst_off - (hlen + skip) of segment byte 0 --
// never dereferenced below dst + dst_off -- so that payload byte `skip` falls on dst + dst_off.  The
// TCP header and the skipped prefix are summed and lie before the stored range.  A record that stores
// nothing (verify only, or skip == data_len) takes the source's own grid (V0 = the segment's address):
// its loads are aligned and it has no stored range.  L2 padding after l3_len is neither read nor
// summed.  Besides that stream every lane reads three header bytes of its record on their own: byte
// 12 (the data offset, all a refused record may read) and bytes 16..17 (the stored field).
//
// Sums: the folded sum is byte-swapped when V0 is odd.  The stored checksum field is part of that sum
// and is taken out by one's complement subtraction (+ 0xffff - field), so `out` holds the
// recomputed value and the compare is exact; the sum cannot be 0 (it holds protocol 6), so the result
// is the representative 1..0xffff that summing with a zeroed field gives.  The pseudo-header
// addresses are summed from the L3 header where it lies, a shifted dword per lane; with F_IP lane 7
// sums the l4_off header bytes with the field masked (an all-zero header must give 0xffff).
//
// Early exit: i >= n, refused records and every other branch on a record's words are uniform over
// the team, so whole teams leave together and no DPP step misses a lane it needs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "recv_common.h"
#include "tcp_recv.h"
#include "team_move.h"

namespace vpcsum {

__global__ __launch_bounds__(256) void k_tcp_recv(const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                 const vpcsum_desc_t* __restrict__ desc,
                                                 const vpcsum_tcprx_t* __restrict__ rx, uint32_t n,
                                                 uint8_t* __restrict__ dst, uint64_t dst_len,
                                                 uint32_t* __restrict__ stored_out, uint32_t* __restrict__ out,
                                                 uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = tid >> 3;            // one team of 8 lanes per record
    const uint32_t tl = threadIdx.x & 7u;
    if (i >= n) return;                     // whole teams leave: no cross-lane step misses a lane it needs

    // the descriptor and the record, the same two loads in every lane of the team
    const Desc d = load_desc(desc + i);
    const u32x4a4_t ra = *(gu32x4a4_t*)(rx + i);
    const uint64_t dst_off = ((uint64_t)ra.y << 32) | ra.x;
    const uint32_t dst_cap = ra.z, skip = ra.w & 0xffffu, ops = (ra.w >> 16) & 0xffu, rsv = ra.w >> 24;

    // a refused record reads its own words and, when the descriptor's bounds allow, the header's byte 12
    bool ok = tcp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len) &&
              tcp_recv_ops_ok(ops, rsv);
    const uint32_t seg_len = d.l3_len - d.l4_off;
    const uintptr_t l3 = (uintptr_t)arena + d.l3_off, seg = l3 + d.l4_off;
    uint32_t hlen = 0, data_len = 0, stored = 0;
    if (ok) {
        const uint32_t b12 = *(gu8_t*)(seg + 12);
        ok = tcp_recv_hdr_ok(seg_len, b12, &hlen, &data_len) &&
             tcp_recv_store_ok(data_len, skip, ops, dst_off, dst_cap, dst_len, &stored);
    }
    if (!ok) {
        if (tl == 0) {
            stored_out[i] = 0u;
            if (out) out[i] = 0u;
            if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
        }
        return;
    }
    // the stored field, as it lies (little-endian domain of the segment's 16-bit words)
    const uint32_t field = (uint32_t) * (gu8_t*)(seg + 16) | ((uint32_t) * (gu8_t*)(seg + 17) << 8);

    // the grid: the destination's when bytes are stored, else the source's own
    const uintptr_t v0 = stored ? (uintptr_t)dst + dst_off - (hlen + skip) : seg;
    const Span sp = make_span(v0, seg, seg_len, stored ? hlen + skip : seg_len);
    const uint32_t ng = (sp.hi + 15u) >> 4;   // seg_len >= 20: at least two groups' worth of bytes
    const uint64_t acc = move_groups<true>(sp, tl, ng);

    // the pseudo-header's addresses, a dword per lane, and the IPv4 header sum: lane 7 (it holds no
    // address dword of an IPv4 packet)
    uint32_t ph = recv_addr_sum(l3, d.l3_ver, tl);
    uint32_t ipw = 0;
    if (tl == 7u && (d.flags & VPCSUM_F_IP)) ipw = recv_ip_header_word(l3, d.l4_off);

    uint32_t ps = fold32(team_sum<8>(fold64(acc)));
    if (v0 & 1u) ps = bswap16(ps);   // the one byte parity of the record
    ph = team_sum<8>(ph);
    ipw = team_sum<8>(ipw);          // lane 7's word in every lane
    if (tl == 0) {
        // protocol 6 and the segment length as the pseudo-header holds them; the stored field out
        const uint64_t total = (uint64_t)ps + ph + (6u << 8) + bswap16(seg_len) + (0xffffu - field);
        const uint32_t l4c = 0xffffu - bswap16(fold64(total));
        uint32_t st = VPCSUM_S_DONE;
        if (bswap16(field) == l4c) st |= VPCSUM_S_L4_OK;
        if (ipw & 0x10000u) st |= VPCSUM_S_IP_OK;
        stored_out[i] = stored;
        if (out) out[i] = (ipw & 0xffffu) | (l4c << 16);
        if (status) status[i] = (uint8_t)st;
    }
}

// A lane per descriptor: the TCP header's first 16 bytes as the 4 or 5 aligned dwords around them.
__global__ __launch_bounds__(256) void k_tcp_digest(const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const vpcsum_desc_t* __restrict__ desc, uint32_t n,
                                                   vpcsum_tcpinfo_t* __restrict__ info) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Desc d = load_desc(desc + i);
    u32x4_t o;
    o.x = o.y = o.z = o.w = 0u;
    if (tcp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len)) {
        const uintptr_t seg = (uintptr_t)arena + d.l3_off + d.l4_off;
        const uint32_t sh = (uint32_t)seg & 3u;
        const uintptr_t a = seg - sh;
        const u32x4a4_t v = *(gu32x4a4_t*)a;
        const uint32_t w4 = sh ? *(gu32_t*)(a + 16) : 0u;   // holds bytes 16 - sh .. 19 - sh: the segment has 20
        const uint32_t d1 = alignbyte(v.z, v.y, sh), d2 = alignbyte(v.w, v.z, sh),
                       d3 = alignbyte(w4, v.w, sh);
        uint32_t hlen = 0, data_len = 0;
        if (tcp_recv_hdr_ok(d.l3_len - d.l4_off, d3 & 0xffu, &hlen, &data_len)) {
            o.x = __builtin_bswap32(d1);
            o.y = __builtin_bswap32(d2);
            o.z = bswap16(d3 >> 16) | (data_len << 16);
            o.w = hlen | (((d3 >> 8) & 0x3fu) << 8);
        }
    }
    *(gwu32x4_t*)(info + i) = o;
}

hipError_t launch_tcp_recv(const uint8_t* arena, uint64_t arena_len, const vpcsum_desc_t* desc, const vpcsum_tcprx_t* rx,
                           uint32_t n, uint8_t* dst, uint64_t dst_len, uint32_t* stored, uint32_t* out, uint8_t* status,
                           hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_tcp_recv, dim3(g), dim3(256), 0, stream, arena, arena_len, desc, rx, n, dst, dst_len, stored, out,
                       status);
    return hipGetLastError();
}

hipError_t launch_tcp_digest(const uint8_t* arena, uint64_t arena_len, const vpcsum_desc_t* desc, uint32_t n,
                             vpcsum_tcpinfo_t* info, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tcp_digest, dim3((n + 255u) / 256u), dim3(256), 0, stream, arena, arena_len, desc, n, info);
    return hipGetLastError();
}

}  // namespace vpcsum
