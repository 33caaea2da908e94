// tcp_build.hip -- k_tcp_build (vpcsum_tcp_build_async): finished TCP data segments from "connection
// header + payload run".  Per record, the payload is read once from the send buffer, written once
// into the TX frame and added to the segment's one's complement accumulator between the two; the
// headers are generated in registers from the 64-B template and stored, with both sums, after the
// team's reduction.  No second kernel, no re-read of the written frame.
//
// Payload: a team of 8 lanes per record (K2's shape for frames) runs team_move.h's mover over it,
// the stored range being all of it: the grid, the source loads, the edges and the sum are described
// there.  No store falls outside [frame_off, frame_off + L).  The TCP header starts at an even
// offset of the segment, so the payload's sum is byte-swapped against the header words' exactly when
// its first address is odd.
//
// Header: lane 0 stores the Ethernet header, lanes 1..3 one 20-byte piece each of the IP and TCP
// headers, every piece from registers in the widest naturally aligned stores its address allows
// (team_move.h store_piece_any).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "tcp_build.h"
#include "team_move.h"

namespace vpcsum {

__global__ __launch_bounds__(256) void k_tcp_build(uint8_t* __restrict__ dst, uint64_t dst_len,
                                                  const uint8_t* __restrict__ src, uint64_t src_len,
                                                  const vpcsum_tcphdr_t* __restrict__ hdrs, uint32_t n_hdr,
                                                  const vpcsum_tcpseg_t* __restrict__ segs, uint32_t n,
                                                  uint32_t* __restrict__ frame_len_out, uint32_t* __restrict__ out,
                                                  uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = tid >> 3;            // one team of 8 lanes per record
    const uint32_t tl = threadIdx.x & 7u;
    if (i >= n) return;                     // whole teams leave: no cross-lane step misses a lane it needs

    // the record (32 B at 8-B alignment), the same two loads in every lane of the team
    const u32x4a4_t ra = *(gu32x4a4_t*)(segs + i);
    const u32x4a4_t rb = *(gu32x4a4_t*)((const uint8_t*)(segs + i) + 16);
    const uint64_t frame_off = ((uint64_t)ra.y << 32) | ra.x, data_off = ((uint64_t)ra.w << 32) | ra.z;
    const uint32_t seq = rb.x, hdr = rb.y, frame_cap = rb.z;
    const uint32_t data_len = rb.w & 0xffffu, flags = (rb.w >> 16) & 0xffu, rsv = rb.w >> 24;

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
        ok = tcp_build_hdr_ok(t) && tcp_build_fits(t, frame_off, data_off, frame_cap, data_len, dst_len, src_len);
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

hipError_t launch_tcp_build(uint8_t* dst, uint64_t dst_len, const uint8_t* src, uint64_t src_len,
                            const vpcsum_tcphdr_t* hdrs, uint32_t n_hdr, const vpcsum_tcpseg_t* segs, uint32_t n,
                            uint32_t* frame_len_out, uint32_t* out, uint8_t* status, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_tcp_build, dim3(g), dim3(256), 0, stream, dst, dst_len, src, src_len, hdrs, n_hdr, segs, n,
                       frame_len_out, out, status);
    return hipGetLastError();
}

}  // namespace vpcsum
