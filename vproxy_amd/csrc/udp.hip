// udp.hip -- k_udp_build (vpcsum_udp_build_async) and k_udp_recv (vpcsum_udp_recv_async): the UDP
// sockets' payload path (UdpOutput.sendUdp, UdpInput.handle), the TCP pair (tcp_frame.h, tcp_recv.hip)
// with UDP's own rules.  A team of 8 lanes per record; the payload goes once through team_move.h's
// mover, read, summed and stored from the same registers.
//
// Build: the payload lies behind an 8-byte header, the stored range is all of it.  The headers are
// generated in registers from the 64-B template and stored, with both sums, after the team's
// reduction: lane 0 the Ethernet header, lanes 1..2 the IP header's 20-byte pieces, the next lane the
// 8 UDP bytes.  A computed UDP sum of 0 is stored as 0xffff.
//
// Receive: the whole segment is laid on the destination's grid through a virtual destination address
// V0 = dst + dst_off - 8 of segment byte 0 -- never dereferenced below dst + dst_off -- so that
// data byte 0 falls on dst + dst_off; the 8 header bytes are summed and lie before the stored range.
// A record that stores nothing (verify only, or a segment of exactly 8 bytes) takes the source's own
// grid.  A segment may be one group (8 bytes inside one 16-B group) or straddle two: the mover's edge
// path takes either.  L2 padding after l3_len is neither read nor summed.  Besides that stream every
// lane reads the stored field (bytes 6..7) on its own.  The UDP length field is summed and not
// consulted.
//
// Sums: the folded sum is byte-swapped when the grid address of segment byte 0 (the build: of the
// payload, 8 bytes on) is odd.  On receive the stored field is part of the sum and is taken out by
// one's complement subtraction (+ 0xffff - field); the sum cannot be 0 (it holds protocol 17), so the
// result is the representative that summing with a zeroed field gives, and UDP's rule (0 -> 0xffff,
// a stored 0 is "no checksum") is applied to that.
//
// Early exit: i >= n, refused records and every other branch on a record's words are uniform over
// the team, so whole teams leave together and no DPP step misses a lane it needs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "recv_common.h"
#include "team_move.h"
#include "udp_build.h"
#include "udp_recv.h"

namespace vpcsum {

__global__ __launch_bounds__(256) void k_udp_build(uint8_t* __restrict__ dst, uint64_t dst_len,
                                                  const uint8_t* __restrict__ src, uint64_t src_len,
                                                  const vpcsum_udphdr_t* __restrict__ hdrs, uint32_t n_hdr,
                                                  const vpcsum_udpdg_t* __restrict__ dgs, uint32_t n,
                                                  uint32_t* __restrict__ frame_len_out, uint32_t* __restrict__ out,
                                                  uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = tid >> 3;            // one team of 8 lanes per record
    const uint32_t tl = threadIdx.x & 7u;
    if (i >= n) return;                     // whole teams leave: no cross-lane step misses a lane it needs

    // the record (32 B at 8-B alignment), the same two loads in every lane of the team
    const u32x4a4_t ra = *(gu32x4a4_t*)(dgs + i);
    const u32x4a4_t rb = *(gu32x4a4_t*)((const uint8_t*)(dgs + i) + 16);
    const uint64_t frame_off = ((uint64_t)ra.y << 32) | ra.x, data_off = ((uint64_t)ra.w << 32) | ra.z;
    const uint32_t hdr = rb.x, frame_cap = rb.y, data_len = rb.z, rsv = rb.w;

    // a refused record loads its own words and, when it names one, its template: nothing else
    bool ok = udp_build_dg_ok(hdr, n_hdr, rsv);
    uint32_t t[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const uint8_t* hp = (const uint8_t*)(hdrs + hdr);
        const u32x4a4_t h0 = *(gu32x4a4_t*)hp, h1 = *(gu32x4a4_t*)(hp + 16), h2 = *(gu32x4a4_t*)(hp + 32),
                        h3 = *(gu32x4a4_t*)(hp + 48);
        t[0] = h0.x; t[1] = h0.y; t[2] = h0.z; t[3] = h0.w;
        t[4] = h1.x; t[5] = h1.y; t[6] = h1.z; t[7] = h1.w;
        t[8] = h2.x; t[9] = h2.y; t[10] = h2.z; t[11] = h2.w;
        t[12] = h3.x; t[13] = h3.y; t[14] = h3.z; t[15] = h3.w;
        ok = udp_build_hdr_ok(t) && udp_build_fits(t, frame_off, data_off, frame_cap, data_len, dst_len, src_len);
    }
    if (!ok) {
        if (tl == 0) {
            frame_len_out[i] = 0u;
            if (out) out[i] = 0u;
            if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
        }
        return;
    }

    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t l2 = tb_l2_len(t), H = udp_build_header_len(t);
    uint8_t* const frame = dst + frame_off;
    uint8_t* const pay = frame + H;

    // the payload, group by group, all of it stored
    const Span sp = make_span((uintptr_t)pay, (uintptr_t)(src + data_off), data_len, 0u);
    const uint32_t ng = data_len ? (sp.hi + 15u) >> 4 : 0u;
    const uint64_t acc = move_groups<false>(sp, tl, ng);
    // the payload's sum in the header words' byte order: its dwords lie on the destination's grid,
    // the UDP header starts on an even byte of the segment
    uint32_t ps = fold32(team_sum<8>(fold64(acc)));
    if ((uintptr_t)pay & 1u) ps = bswap16(ps);

    // the header: every lane of the team holds all of it
    UdpBuildWords w;
    udp_build_words(t, data_len, w);
    const uint32_t ip_field = v4 ? 0xffffu - fold64(udp_build_ip_header_sum(w)) : 0u;
    const uint32_t l4_field = udp_build_l4_field(fold64(udp_build_l4_header_sum(t, w, data_len) + ps));
    udp_build_set_sums(w, v4, ip_field, l4_field);

    if (tl == 0) {
        if (l2) {
            store_piece_any<14>(frame, Piece{w.eth[0], w.eth[1], w.eth[2], w.eth[3], 0u});
        }
        frame_len_out[i] = H + data_len;
        if (out) out[i] = bswap16(ip_field) | (bswap16(l4_field) << 16);
        if (status) status[i] = (uint8_t)VPCSUM_S_DONE;
    } else if (tl == 1) {
        // 20-byte pieces of the IP header, a lane each, then the 8 UDP bytes -- IPv4: ip, udp; IPv6:
        // ip[0..4], ip[5..9], udp.  (One branch per piece, every word under a compile-time index.)
        store_piece_any<20>(frame + l2, Piece{w.ip[0], w.ip[1], w.ip[2], w.ip[3], w.ip[4]});
    } else if (tl == 2 && !v4) {
        store_piece_any<20>(frame + l2 + 20u, Piece{w.ip[5], w.ip[6], w.ip[7], w.ip[8], w.ip[9]});
    } else if (tl == (v4 ? 2u : 3u)) {
        store_piece_any<8>(frame + l2 + (v4 ? 20u : 40u), Piece{w.udp[0], w.udp[1], 0u, 0u, 0u});
    }
}

__global__ __launch_bounds__(256) void k_udp_recv(const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                 const vpcsum_desc_t* __restrict__ desc,
                                                 const vpcsum_udprx_t* __restrict__ rx, uint32_t n,
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
    const uint32_t dst_cap = ra.z, ops = ra.w & 0xffu, rsv = ra.w >> 8;

    // a refused record reads its own words: nothing of the arena
    const uint32_t seg_len = d.l3_len - d.l4_off;
    uint32_t stored = 0;
    const bool ok = udp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len) &&
                    udp_recv_ops_ok(ops, rsv) && udp_recv_store_ok(seg_len, ops, dst_off, dst_cap, dst_len, &stored);
    if (!ok) {
        if (tl == 0) {
            stored_out[i] = 0u;
            if (out) out[i] = 0u;
            if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
        }
        return;
    }
    const uintptr_t l3 = (uintptr_t)arena + d.l3_off, seg = l3 + d.l4_off;
    // the stored field, as it lies (little-endian domain of the segment's 16-bit words)
    const uint32_t field = (uint32_t) * (gu8_t*)(seg + 6) | ((uint32_t) * (gu8_t*)(seg + 7) << 8);

    // the grid: the destination's when bytes are stored, else the source's own
    const uintptr_t v0 = stored ? (uintptr_t)dst + dst_off - kUdpHeader : seg;
    const Span sp = make_span(v0, seg, seg_len, stored ? kUdpHeader : seg_len);
    const uint32_t ng = (sp.hi + 15u) >> 4;   // seg_len >= 8: at least one group
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
        // protocol 17 and the segment length as the pseudo-header holds them; the stored field out
        const uint64_t total = (uint64_t)ps + ph + (17u << 8) + bswap16(seg_len) + (0xffffu - field);
        const uint32_t l4c = udp_recv_l4c(0xffffu - bswap16(fold64(total)));
        uint32_t st = VPCSUM_S_DONE | udp_recv_l4_status(bswap16(field), 0xffffu - bswap16(fold64(total)));
        if (ipw & 0x10000u) st |= VPCSUM_S_IP_OK;
        stored_out[i] = stored;
        if (out) out[i] = (ipw & 0xffffu) | (l4c << 16);
        if (status) status[i] = (uint8_t)st;
    }
}

hipError_t launch_udp_build(uint8_t* dst, uint64_t dst_len, const uint8_t* src, uint64_t src_len,
                            const vpcsum_udphdr_t* hdrs, uint32_t n_hdr, const vpcsum_udpdg_t* dgs, uint32_t n,
                            uint32_t* frame_len_out, uint32_t* out, uint8_t* status, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_udp_build, dim3(g), dim3(256), 0, stream, dst, dst_len, src, src_len, hdrs, n_hdr, dgs, n,
                       frame_len_out, out, status);
    return hipGetLastError();
}

hipError_t launch_udp_recv(const uint8_t* arena, uint64_t arena_len, const vpcsum_desc_t* desc, const vpcsum_udprx_t* rx,
                           uint32_t n, uint8_t* dst, uint64_t dst_len, uint32_t* stored, uint32_t* out, uint8_t* status,
                           hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_udp_recv, dim3(g), dim3(256), 0, stream, arena, arena_len, desc, rx, n, dst, dst_len, stored, out,
                       status);
    return hipGetLastError();
}

}  // namespace vpcsum
