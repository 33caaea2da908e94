// tcp_frame.h -- the body of the TCP segment build, held once: what a team of 8 lanes does once its
// frame's record is known.  k_tcp_build (tcp_build.hip) reads the record from memory, k_tcp_build_bursts
// (tcp_burst.hip) derives it from the frame's burst; both call tcp_build_frame.
//
// Payload: team_move.h's mover over it, the stored range being all of it: the grid, the source loads,
// the edges and the sum are described there.  No store falls outside [frame_off, frame_off + L).  The
// TCP header starts at an even offset of the segment, so the payload's sum is byte-swapped against
// the header words' exactly when its first address is odd.
//
// Header: lane 0 stores the Ethernet header, lanes 1..3 one 20-byte piece each of the IP and TCP
// headers, every piece from registers in the widest naturally aligned stores its address allows
// (team_move.h store_piece_any).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "tcp_build.h"
#include "team_move.h"

namespace vpcsum {

// What a refused frame reports; not one byte of the arena is written
__device__ __forceinline__ void tcp_build_refuse(uint32_t i, uint32_t tl, uint32_t* frame_len_out,
                                                 uint32_t* out, uint8_t* status) {
    if (tl == 0) {
        frame_len_out[i] = 0u;
        if (out) out[i] = 0u;
        if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
    }
}

// Frame i from its record's fields, by the team's lane tl.  also_ok(t): what the caller's rule asks
// of the accepted template's words besides the record's own checks (a burst: tcp_burst_ok), evaluated
// before anything but the record and the template is read.
template <class AlsoOk>
__device__ __forceinline__ void tcp_build_frame(uint8_t* dst, uint64_t dst_len, const uint8_t* src,
                                                uint64_t src_len, const vpcsum_tcphdr_t* hdrs, uint32_t n_hdr,
                                                uint32_t i, uint32_t tl, uint64_t frame_off, uint64_t data_off, uint32_t seq,
                                                uint32_t hdr, uint32_t frame_cap, uint32_t data_len, uint32_t flags,
                                                uint32_t rsv, uint32_t* frame_len_out, uint32_t* out,
                                                uint8_t* status, AlsoOk also_ok) {
    // a refused record loads its own words and, when it names one, its template: nothing else
    bool ok = tcp_build_seg_ok(hdr, n_hdr, flags, rsv);
    uint32_t t[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const uint8_t* hp = (const uint8_t*)(hdrs + hdr);
        const u32x4a4_t h0 = *(gu32x4a4_t*)hp, h1 = *(gu32x4a4_t*)(hp + 16), h2 = *(gu32x4a4_t*)(hp + 32),
                        h3 = *(gu32x4a4_t*)(hp + 48);
        t[0] = h0.x; t[1] = h0.y; t[2] = h0.z; t[3] = h0.w;
        t[4] = h1.x; t[5] = h1.y; t[6] = h1.z; t[7] = h1.w;
        t[8] = h2.x; t[9] = h2.y; t[10] = h2.z; t[11] = h2.w;
        t[12] = h3.x; t[13] = h3.y; t[14] = h3.z; t[15] = h3.w;
        ok = tcp_build_hdr_ok(t) && also_ok(t) &&
             tcp_build_fits(t, frame_off, data_off, frame_cap, data_len, dst_len, src_len);
    }
    if (!ok) {
        tcp_build_refuse(i, tl, frame_len_out, out, status);
        return;
    }

    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t l2 = tb_l2_len(t), H = tcp_build_header_len(t);
    uint8_t* const frame = dst + frame_off;
    uint8_t* const pay = frame + H;

    // the payload, group by group, all of it stored
    const Span sp = make_span((uintptr_t)pay, (uintptr_t)(src + data_off), data_len, 0u);
    const uint32_t ng = data_len ? (sp.hi + 15u) >> 4 : 0u;
    const uint64_t acc = move_groups<false>(sp, tl, ng);
    // the payload's sum in the header words' byte order: its dwords lie on the destination's grid,
    // the TCP header starts on an even byte of the segment
    uint32_t ps = fold32(team_sum<8>(fold64(acc)));
    if ((uintptr_t)pay & 1u) ps = bswap16(ps);

    // the header: every lane of the team holds all of it
    TcpBuildWords w;
    tcp_build_words(t, seq, data_len, flags, w);
    const uint32_t ip_field = v4 ? 0xffffu - fold64(tcp_build_ip_header_sum(w)) : 0u;
    const uint32_t l4_field = 0xffffu - fold64(tcp_build_l4_header_sum(t, w, data_len) + ps);
    tcp_build_set_sums(w, v4, ip_field, l4_field);

    if (tl == 0) {
        if (l2) {
            store_piece_any<14>(frame, Piece{w.eth[0], w.eth[1], w.eth[2], w.eth[3], 0u});
        }
        frame_len_out[i] = H + data_len;
        if (out) out[i] = bswap16(ip_field) | (bswap16(l4_field) << 16);
        if (status) status[i] = (uint8_t)VPCSUM_S_DONE;
    } else if (tl == 1) {
        // 20-byte pieces of IP ‖ TCP, a lane each -- IPv4: ip, tcp; IPv6: ip[0..4], ip[5..9], tcp.  (One
        // branch per piece, every word under a compile-time index.)
        store_piece_any<20>(frame + l2, Piece{w.ip[0], w.ip[1], w.ip[2], w.ip[3], w.ip[4]});
    } else if (tl == 2 && !v4) {
        store_piece_any<20>(frame + l2 + 20u, Piece{w.ip[5], w.ip[6], w.ip[7], w.ip[8], w.ip[9]});
    } else if (tl == (v4 ? 2u : 3u)) {
        store_piece_any<20>(frame + l2 + (v4 ? 20u : 40u), Piece{w.tcp[0], w.tcp[1], w.tcp[2], w.tcp[3], w.tcp[4]});
    }
}

}  // namespace vpcsum
