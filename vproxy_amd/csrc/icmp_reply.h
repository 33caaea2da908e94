// icmp_reply.h -- the rules of the ICMP replies that are not HIP (vpcsum_icmp_reply_async,
// include/vpcsum.h): which records are refused, the message length M and the frame length L, and the
// header bytes without their two sums, from a parse descriptor, a template (vpcsum_icmphdr_t) and a
// record (vpcsum_icmprp_t).  Plain C++, shared by the kernel (icmp.hip), the host entry (api.cpp) and
// a stand-alone test (tests/cpp/icmp_rules_test.cpp).
//
// The three replies of the reference end in SwitchUtils.buildEtherIpIcmpPacket (SwitchUtils.java:
// 202-241): IcmpInput.respondIcmpPong (echo), IcmpPortUnreachableOutput.handle, IPInputRoute.
// respondIcmpTimeExceeded.  The template is the TCP build's 64 bytes, held as the same 16 little-endian
// dwords (tcp_build.h); Ethernet and IP are tcp_build.h's tb_* helpers with protocol 1 / 58 and an
// 8-byte L4 header.  What is ICMP's own: a template's ports, ack and window (t[12], t[13], the low
// half of t[14]) must be 0; the message is type | code | sum and either the request's bytes from 4 on
// (echo) or four zero bytes and the first q bytes of the request's IP packet (the two errors); ICMPv6
// sums the pseudo-header of the template's addresses, ICMPv4 none; a computed 0x0000 is stored as it
// is and an all-zero message stores 0xffff -- both fall out of folding an exact integer sum.
//
// The rule runs in steps, so that a refused record reads as little as the step that refuses it
// needs: the record's own words, the template, the descriptor with the record's kind and the
// destination (nothing of the arena), then the one type byte where the kind asks for it.
#pragma once
#include <stdint.h>

#include "tcp_build.h"
#include "udp_build.h"
#include "vpcsum.h"

namespace vpcsum {

static_assert(sizeof(vpcsum_icmphdr_t) == 64 && sizeof(vpcsum_icmprp_t) == 24, "vpcsum.h: template 64 B, record 24 B");

constexpr uint32_t kIcmpHeader = 8;          // type, code, sum, and the echo's id / seq or the errors' unused dword
constexpr uint32_t kIcmpQuotePastHeader = 64;   // the errors quote headerLen + 64 bytes at the most
constexpr uint32_t kIcmpReplyMaxHeader = 62;    // 14 + 40 + 8

// The record's own words: a template that exists, a kind that exists, rsv (its seven bytes as the high
// three of one dword and the next) 0.  Checked before the template is read.
VPC_TB_FN bool icmp_reply_rp_ok(uint32_t hdr, uint32_t n_hdr, uint32_t kind, uint32_t rsv_lo, uint32_t rsv_hi) {
    return hdr < n_hdr && kind >= VPCSUM_ICMP_ECHO_REPLY && kind <= VPCSUM_ICMP_TIME_EXCEEDED && rsv_lo == 0 && rsv_hi == 0;
}

// The template: one the UDP build accepts whose ports (bytes 48..51) are 0 too.
VPC_TB_FN bool icmp_reply_hdr_ok(const uint32_t (&t)[16]) { return udp_build_hdr_ok(t) && t[12] == 0; }

// The descriptor, whatever the kind: IPv4 / IPv6 of the template's version, no F_L4P / F_RAW / F_PRE,
// F_IP only on IPv4, an L4 offset vpcsum_compute_async takes, the packet inside the arena (no wrap).
VPC_TB_FN bool icmp_reply_desc_ok(uint64_t l3_off, uint32_t l3_len, uint32_t l4_off, uint32_t l3_ver, uint32_t flags,
                                  uint32_t tmpl_ver, uint64_t arena_len) {
    if (l3_ver != 4u && l3_ver != 6u) return false;
    if (l3_ver != tmpl_ver) return false;
    if (flags & (VPCSUM_F_L4P | VPCSUM_F_RAW | VPCSUM_F_PRE)) return false;
    if ((flags & VPCSUM_F_IP) && l3_ver != 4u) return false;
    if (l4_off > l3_len) return false;
    if (l3_ver == 4u ? (l4_off < 20u || (l4_off & 3u)) : l4_off < 40u) return false;
    if (l3_off > arena_len || (uint64_t)l3_len > arena_len - l3_off) return false;
    return true;
}

// The kind against an accepted descriptor.  Echo: an ICMP message of its own family (IcmpInput.java:
// 40-52 drops the other) with F_L4, at least the 8 bytes IcmpPacket.from asks for.  Port unreachable:
// UDP (UdpInput's miss branch is its only caller).  Time exceeded: any packet.
VPC_TB_FN bool icmp_reply_kind_ok(uint32_t kind, uint32_t l3_ver, uint32_t l4_proto, uint32_t flags, uint32_t seg_len) {
    if (kind == VPCSUM_ICMP_ECHO_REPLY)
        return (flags & VPCSUM_F_L4) && l4_proto == (l3_ver == 4u ? 1u : 58u) && seg_len >= kIcmpHeader;
    if (kind == VPCSUM_ICMP_PORT_UNREACH) return l4_proto == 17u;
    return true;
}

// The quoted bytes of an error: min(l3_len, l4_off + 64) from the IP header on (headerLen + 64, the
// rebuilt header being l4_off bytes long)
VPC_TB_FN uint32_t icmp_reply_quote_len(uint32_t l3_len, uint32_t l4_off) {
    const uint32_t cap = l4_off + kIcmpQuotePastHeader;
    return l3_len < cap ? l3_len : cap;
}

// M, the ICMP message length, of an accepted descriptor and kind
VPC_TB_FN uint32_t icmp_reply_msg_len(uint32_t kind, uint32_t l3_len, uint32_t l4_off) {
    return kind == VPCSUM_ICMP_ECHO_REPLY ? l3_len - l4_off : kIcmpHeader + icmp_reply_quote_len(l3_len, l4_off);
}

// L of an accepted template and a message of M >= 8 bytes
VPC_TB_FN uint32_t icmp_reply_frame_len(const uint32_t (&t)[16], uint32_t M) { return tb_header_len(t, 0u) + M; }

// Whether the reply fits: the chunk's room, the destination (no wrap).  The length field always holds
// it: an echo's M is seg_len <= l3_len - (20 | 40) of a 16-bit l3_len, an error's at most 8 + l4_off
// + 64, so 20 + M (IPv4) and M (IPv6) stay within 65,535 and nothing here overflows 32 bits.
VPC_TB_FN bool icmp_reply_fits(const uint32_t (&t)[16], uint32_t M, uint64_t frame_off, uint32_t frame_cap, uint64_t dst_len) {
    const uint32_t L = icmp_reply_frame_len(t, M);
    if (L > frame_cap) return false;
    if (frame_off > dst_len || (uint64_t)L > dst_len - frame_off) return false;
    return true;
}

// Whether the kind consults byte 0 of the segment, and what it asks of it.  Echo: the request's type,
// 8 / 128 (IcmpInput.java:72, 89).  Time exceeded: an ICMPv6 segment of at least one byte must not be
// a neighbour solicitation / advertisement (IPInputRoute.java:64-75 drops those before the hop check).
VPC_TB_FN bool icmp_reply_reads_type(uint32_t kind, uint32_t l3_ver, uint32_t l4_proto, uint32_t seg_len) {
    if (kind == VPCSUM_ICMP_ECHO_REPLY) return true;
    return kind == VPCSUM_ICMP_TIME_EXCEEDED && l3_ver == 6u && l4_proto == 58u && seg_len >= 1u;
}
VPC_TB_FN bool icmp_reply_type_ok(uint32_t kind, uint32_t l3_ver, uint32_t type) {
    if (kind == VPCSUM_ICMP_ECHO_REPLY) return type == (l3_ver == 4u ? 8u : 128u);
    return type != 135u && type != 136u;
}

// The reply's type | code << 8, the first little-endian halfword of the message
VPC_TB_FN uint32_t icmp_reply_type_code(uint32_t kind, bool v4) {
    if (kind == VPCSUM_ICMP_ECHO_REPLY) return v4 ? 0u : 129u;                       // code 0 whatever the request's
    if (kind == VPCSUM_ICMP_PORT_UNREACH) return v4 ? (3u | (3u << 8)) : (1u | (4u << 8));
    return v4 ? 11u : 3u;
}

// The header's words, sums left 0 (tcp_build.h TcpBuildWords' layout, with 2 ICMP words; an echo
// reply's second word is the request's and is not stored from here)
struct IcmpReplyWords {
    uint32_t eth[4];
    uint32_t ip[10];
    uint32_t icmp[2];
};

VPC_TB_FN void icmp_reply_words(const uint32_t (&t)[16], uint32_t kind, uint32_t M, IcmpReplyWords& w) {
    const bool v4 = tb_l3_ver(t) == 4;
    tb_eth_ip_words(t, v4 ? 1u : 58u, kIcmpHeader, M - kIcmpHeader, w.eth, w.ip);
    w.icmp[0] = icmp_reply_type_code(kind, v4);
    w.icmp[1] = 0;
}

// The one's complement sum, in the words' own (little-endian) domain, of what the ICMP sum covers
// besides the bytes that come out of the request: type and code, and for ICMPv6 the pseudo-header of
// the template's addresses (IcmpPacket.updateChecksumWithIPv6, IcmpPacket.java:124-135: next header
// 58, the message length).  ICMPv4 has no pseudo-header.  Not folded.
VPC_TB_FN uint64_t icmp_reply_l4_header_sum(const uint32_t (&t)[16], const IcmpReplyWords& w, uint32_t M) {
    const uint64_t s = w.icmp[0];
    return tb_l3_ver(t) == 4 ? s : tb_add_pseudo_sum(s, t, 58u, kIcmpHeader, M - kIcmpHeader);
}

VPC_TB_FN uint64_t icmp_reply_ip_header_sum(const IcmpReplyWords& w) {
    return (uint64_t)w.ip[0] + w.ip[1] + w.ip[2] + w.ip[3] + w.ip[4];
}

// The ICMP field as it lies in the words, from the folded little-endian sum of everything it covers
// (0 only when every summed byte is 0): its complement, nothing else -- an all-zero message gives
// 0xffff, a sum of 0xffff gives 0x0000, as Utils.calculateChecksum does.
VPC_TB_FN uint32_t icmp_reply_l4_field(uint32_t folded) { return 0xffffu - folded; }

// Put the sums in: the 16 bits as they lie in the words
VPC_TB_FN void icmp_reply_set_sums(IcmpReplyWords& w, bool v4, uint32_t ip_field, uint32_t l4_field) {
    if (v4) w.ip[2] |= ip_field << 16;
    w.icmp[0] |= l4_field << 16;
}

#ifndef __HIP_DEVICE_COMPILE__
// Host: the whole rule on a descriptor, a record and its template (NULL when the record names none:
// hdr >= n_hdr), the segment's byte 0 read through `type_at` only when every other step passed and the
// kind asks for it.  What the kernel decides, for the stand-alone test and host callers.
struct IcmpReplyPlan { uint32_t M, L, q; };
template <class TypeAt>
inline bool icmp_reply_plan(const vpcsum_desc_t& d, const vpcsum_icmprp_t& r, const vpcsum_icmphdr_t* hdrs, uint32_t n_hdr,
                            uint64_t arena_len, uint64_t dst_len, TypeAt type_at, IcmpReplyPlan* p) {
    *p = IcmpReplyPlan{0, 0, 0};
    const uint32_t rsv_lo = (uint32_t)r.rsv[0] | ((uint32_t)r.rsv[1] << 8) | ((uint32_t)r.rsv[2] << 16);
    const uint32_t rsv_hi = (uint32_t)r.rsv[3] | ((uint32_t)r.rsv[4] << 8) | ((uint32_t)r.rsv[5] << 16) | ((uint32_t)r.rsv[6] << 24);
    if (!icmp_reply_rp_ok(r.hdr, n_hdr, r.kind, rsv_lo, rsv_hi)) return false;
    uint32_t t[16];
    tcp_build_template_words(hdrs[r.hdr], t);
    if (!icmp_reply_hdr_ok(t)) return false;
    if (!icmp_reply_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.flags, tb_l3_ver(t), arena_len)) return false;
    const uint32_t seg_len = (uint32_t)d.l3_len - d.l4_off;
    if (!icmp_reply_kind_ok(r.kind, d.l3_ver, d.l4_proto, d.flags, seg_len)) return false;
    const uint32_t M = icmp_reply_msg_len(r.kind, d.l3_len, d.l4_off);
    if (!icmp_reply_fits(t, M, r.frame_off, r.frame_cap, dst_len)) return false;
    if (icmp_reply_reads_type(r.kind, d.l3_ver, d.l4_proto, seg_len) &&
        !icmp_reply_type_ok(r.kind, d.l3_ver, type_at(d.l3_off + d.l4_off)))
        return false;
    *p = IcmpReplyPlan{M, icmp_reply_frame_len(t, M),
                       r.kind == VPCSUM_ICMP_ECHO_REPLY ? 0u : icmp_reply_quote_len(d.l3_len, d.l4_off)};
    return true;
}

// Host: the header bytes (sums as the words hold them) as they lie in the frame; returns their count
inline uint32_t icmp_reply_header_bytes(const IcmpReplyWords& w, const uint32_t (&t)[16], uint8_t* out) {
    return tb_header_bytes(w.eth, w.ip, w.icmp, kIcmpHeader, t, out);
}
#endif

}  // namespace vpcsum
