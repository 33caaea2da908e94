// icmp.hip -- k_icmp_reply (vpcsum_icmp_reply_async): the replies the vswitch generates itself --
// echo (IcmpInput.respondIcmpPong), port unreachable (IcmpPortUnreachableOutput.handle), time
// exceeded (IPInputRoute.respondIcmpTimeExceeded) -- as finished Ethernet / IP / ICMP frames, each
// byte-equal to getRawPacket(0) of what SwitchUtils.buildEtherIpIcmpPacket builds.  A source named by
// a parse descriptor as in the receives (recv_common.h), headers generated from the 64-B template as
// in the builds (icmp_reply.h over tcp_build.h), one pass of team_move.h's mover between the two.  A
// team of 8 lanes per record.
//
// Echo: the request's segment is laid on the reply's grid with segment byte 0 at the reply's ICMP
// byte 0, summed whole and stored from byte 4 on.  The first dword (type, code, field) is read once
// more by every lane and taken out of lane 0's (and, when it straddles the first group, lane 1's)
// integer accumulator before anything is folded -- an exact subtraction, so the sum of bytes [4,
// seg_len) is 0 only when they are all 0 and the IPv4 echo of an all-zero body stores 0xffff as Java
// does, where one's complement subtraction would store 0x0000.  The same sum gives the request's
// verdict (what vpcsum_compute_async writes under VPCSUM_MODE_VERIFY: + the request's type and code,
// for ICMPv6 the pseudo-header of the request's addresses) and the reply's field (+ the reply's type,
// for ICMPv6 the pseudo-header of the template's addresses).
//
// Errors: the first q = min(l3_len, l4_off + 64) bytes of the IP packet are laid 8 bytes behind the
// reply's ICMP byte 0, all of them stored.
//
// The headers are stored, with both sums, after the team's reduction: lane 0 the Ethernet header,
// lanes 1..2 the IP header's 20-byte pieces, the next lane the ICMP header (an echo's 4 bytes, an
// error's 8).
//
// Early exit: i >= n, refused records and every other branch on a record's words are uniform over
// the team, so whole teams leave together and no DPP step misses a lane it needs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "icmp_reply.h"
#include "internal.h"
#include "recv_common.h"
#include "team_move.h"

namespace vpcsum {

// source and destination may be one allocation (an XDP umem holds both rings' chunks): no __restrict__
// on the two arenas
__global__ __launch_bounds__(256) void k_icmp_reply(const uint8_t* arena, uint64_t arena_len,
                                                   const vpcsum_desc_t* __restrict__ desc,
                                                   const vpcsum_icmphdr_t* __restrict__ hdrs, uint32_t n_hdr,
                                                   const vpcsum_icmprp_t* __restrict__ rps, uint32_t n, uint8_t* dst,
                                                   uint64_t dst_len, uint32_t* __restrict__ frame_len_out,
                                                   uint32_t* __restrict__ csum_out, uint32_t* __restrict__ out,
                                                   uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = tid >> 3;            // one team of 8 lanes per record
    const uint32_t tl = threadIdx.x & 7u;
    if (i >= n) return;                     // whole teams leave: no cross-lane step misses a lane it needs

    // the descriptor and the record (24 B at 8-B alignment), the same loads in every lane of the team
    const Desc d = load_desc(desc + i);
    const u32x4a4_t ra = *(gu32x4a4_t*)(rps + i);
    const u32x2a4_t rb = *(gu32x2a4_t*)((const uint8_t*)(rps + i) + 16);
    const uint64_t frame_off = ((uint64_t)ra.y << 32) | ra.x;
    const uint32_t hdr = ra.z, frame_cap = ra.w, kind = rb.x & 0xffu;

    // a refused record loads its own words and, when it names one, its template; of the arena the one
    // type byte, and that only when nothing else refuses it
    const uint32_t seg_len = d.l3_len - d.l4_off;
    uint32_t M = 0;
    bool ok = icmp_reply_rp_ok(hdr, n_hdr, kind, rb.x >> 8, rb.y);
    uint32_t t[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const uint8_t* hp = (const uint8_t*)(hdrs + hdr);
        const u32x4a4_t h0 = *(gu32x4a4_t*)hp, h1 = *(gu32x4a4_t*)(hp + 16), h2 = *(gu32x4a4_t*)(hp + 32),
                        h3 = *(gu32x4a4_t*)(hp + 48);
        t[0] = h0.x; t[1] = h0.y; t[2] = h0.z; t[3] = h0.w;
        t[4] = h1.x; t[5] = h1.y; t[6] = h1.z; t[7] = h1.w;
        t[8] = h2.x; t[9] = h2.y; t[10] = h2.z; t[11] = h2.w;
        t[12] = h3.x; t[13] = h3.y; t[14] = h3.z; t[15] = h3.w;
        ok = icmp_reply_hdr_ok(t) && icmp_reply_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.flags, tb_l3_ver(t), arena_len) &&
             icmp_reply_kind_ok(kind, d.l3_ver, d.l4_proto, d.flags, seg_len);
        if (ok) {
            M = icmp_reply_msg_len(kind, d.l3_len, d.l4_off);
            ok = icmp_reply_fits(t, M, frame_off, frame_cap, dst_len);
        }
    }
    const uintptr_t l3 = (uintptr_t)arena + d.l3_off, seg = l3 + d.l4_off;
    if (ok && icmp_reply_reads_type(kind, d.l3_ver, d.l4_proto, seg_len))
        ok = icmp_reply_type_ok(kind, d.l3_ver, *(gu8_t*)seg);
    if (!ok) {
        if (tl == 0) {
            frame_len_out[i] = 0u;
            if (csum_out) csum_out[i] = 0u;
            if (out) out[i] = 0u;
            if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
        }
        return;
    }

    const bool v4 = d.l3_ver == 4u;
    const bool echo = kind == VPCSUM_ICMP_ECHO_REPLY;
    const uint32_t l2 = tb_l2_len(t), ih = v4 ? 20u : 40u;
    uint8_t* const frame = dst + frame_off;
    uint8_t* const icmp = frame + l2 + ih;   // the reply's ICMP byte 0

    // body: the folded sum, in the message's own 16-bit word order, of what the reply takes out of
    // the request -- segment bytes [4, seg_len), or the q quoted bytes.  0 only when they are all 0.
    uint32_t body, req_out = 0, req_st = VPCSUM_S_DONE;
    if (echo) {
        const uint32_t w0 = load_shifted(seg);   // type | code << 8 | field << 16, as it lies
        const Span sp = make_span((uintptr_t)icmp, seg, seg_len, 4u);
        const uint32_t ng = (sp.hi + 15u) >> 4;   // seg_len >= 8: at least one group
        uint64_t acc = move_groups<true>(sp, tl, ng);
        // the first dword out of the accumulators that hold it, exactly: it lies on grid bytes [lo, lo + 4),
        // the low part in grid dword lo >> 2 and, when lo & 3, the rest in the next, which is group 1's
        // first when lo > 12
        const uint32_t r = sp.lo & 3u, j = sp.lo >> 2;
        const uint32_t part_lo = w0 << (8u * r), part_hi = r ? w0 >> (32u - 8u * r) : 0u;
        if (tl == 0u) acc -= (uint64_t)part_lo + (j < 3u ? part_hi : 0u);
        if (tl == 1u && j == 3u) acc -= part_hi;

        // the request's pseudo-header addresses (ICMPv6), a dword per lane, and its IPv4 header sum: lane 7
        uint32_t ph = v4 ? 0u : recv_addr_sum(l3, d.l3_ver, tl);
        uint32_t ipw = 0;
        if (tl == 7u && (d.flags & VPCSUM_F_IP)) ipw = recv_ip_header_word(l3, d.l4_off);

        body = fold32(team_sum<8>(fold64(acc)));
        if ((uintptr_t)icmp & 1u) body = bswap16(body);   // the one byte parity of the record
        ph = team_sum<8>(ph);
        ipw = team_sum<8>(ipw);          // lane 7's word in every lane

        // the request's verdict: its sum with the field taken as 0 -- an exact 0 for an all-zero ICMPv4
        // message, hence 0xffff
        uint64_t total = (uint64_t)body + (w0 & 0xffffu);
        if (!v4) total += (uint64_t)ph + (58u << 8) + bswap16(seg_len);
        const uint32_t l4c = 0xffffu - bswap16(fold64(total));
        if (bswap16(w0 >> 16) == l4c) req_st |= VPCSUM_S_L4_OK;
        if (ipw & 0x10000u) req_st |= VPCSUM_S_IP_OK;
        req_out = (ipw & 0xffffu) | (l4c << 16);
    } else {
        const uint32_t q = M - kIcmpHeader;   // at least the IP header's bytes
        const Span sp = make_span((uintptr_t)(icmp + kIcmpHeader), l3, q, 0u);
        const uint32_t ng = (sp.hi + 15u) >> 4;
        const uint64_t acc = move_groups<false>(sp, tl, ng);
        body = fold32(team_sum<8>(fold64(acc)));
        if ((uintptr_t)icmp & 1u) body = bswap16(body);   // the quote starts 8 bytes on: the same parity
    }

    // the header: every lane of the team holds all of it
    IcmpReplyWords w;
    icmp_reply_words(t, kind, M, w);
    const uint32_t ip_field = v4 ? 0xffffu - fold64(icmp_reply_ip_header_sum(w)) : 0u;
    const uint32_t l4_field = icmp_reply_l4_field(fold64(icmp_reply_l4_header_sum(t, w, M) + body));
    icmp_reply_set_sums(w, v4, ip_field, l4_field);

    if (tl == 0) {
        if (l2) {
            store_piece_any<14>(frame, Piece{w.eth[0], w.eth[1], w.eth[2], w.eth[3], 0u});
        }
        frame_len_out[i] = l2 + ih + M;
        if (csum_out) csum_out[i] = bswap16(ip_field) | (bswap16(l4_field) << 16);
        if (out) out[i] = req_out;
        if (status) status[i] = (uint8_t)req_st;
    } else if (tl == 1) {
        // 20-byte pieces of the IP header, a lane each, then the ICMP header -- IPv4: ip, icmp; IPv6:
        // ip[0..4], ip[5..9], icmp.  (One branch per piece, every word under a compile-time index.)
        store_piece_any<20>(frame + l2, Piece{w.ip[0], w.ip[1], w.ip[2], w.ip[3], w.ip[4]});
    } else if (tl == 2 && !v4) {
        store_piece_any<20>(frame + l2 + 20u, Piece{w.ip[5], w.ip[6], w.ip[7], w.ip[8], w.ip[9]});
    } else if (tl == (v4 ? 2u : 3u)) {
        // an echo's bytes 4..7 are the request's and came through the mover
        if (echo) store_piece_any<4>(icmp, Piece{w.icmp[0], 0u, 0u, 0u, 0u});
        else store_piece_any<8>(icmp, Piece{w.icmp[0], w.icmp[1], 0u, 0u, 0u});
    }
}

hipError_t launch_icmp_reply(const uint8_t* arena, uint64_t arena_len, const vpcsum_desc_t* desc, const vpcsum_icmphdr_t* hdrs,
                             uint32_t n_hdr, const vpcsum_icmprp_t* rps, uint32_t n, uint8_t* dst, uint64_t dst_len,
                             uint32_t* frame_len_out, uint32_t* csum_out, uint32_t* out, uint8_t* status, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_icmp_reply, dim3(g), dim3(256), 0, stream, arena, arena_len, desc, hdrs, n_hdr, rps, n, dst, dst_len,
                       frame_len_out, csum_out, out, status);
    return hipGetLastError();
}

}  // namespace vpcsum
