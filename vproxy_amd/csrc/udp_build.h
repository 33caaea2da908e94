// udp_build.h -- the rules of the UDP datagram build that are not HIP (vpcsum_udp_build_async,
// include/vpcsum.h): which records are refused, the frame length L, and the header bytes without
// their two sums, from a template (vpcsum_udphdr_t) and a record (vpcsum_udpdg_t).  Plain C++, shared
// by the kernel (udp.hip), the host entry (api.cpp) and a stand-alone test
// (tests/cpp/udp_rules_test.cpp).
//
// The template is the TCP build's 64 bytes, held as the same 16 little-endian dwords (tcp_build.h);
// Ethernet, IP and the pseudo-header are tcp_build.h's tb_* helpers with protocol 17 and an 8-byte
// L4 header.  What is UDP's own: a template's ack / window (t[13], the low half of t[14]) must be 0,
// the record has no seq / flags and a 32-bit data_len, the header is ports | length | sum, and a
// computed sum of 0 is stored as 0xffff.
#pragma once
#include <stdint.h>

#include "tcp_build.h"
#include "vpcsum.h"

namespace vpcsum {

static_assert(sizeof(vpcsum_udphdr_t) == 64 && sizeof(vpcsum_udpdg_t) == 32, "vpcsum.h: template 64 B, record 32 B");

constexpr uint32_t kUdpHeader = 8;
constexpr uint32_t kUdpBuildMaxHeader = 62;   // 14 + 40 + 8

// The record's own words: rsv 0, a template that exists.  Checked before the template is read.
VPC_TB_FN bool udp_build_dg_ok(uint32_t hdr, uint32_t n_hdr, uint32_t rsv) { return hdr < n_hdr && rsv == 0; }

// The template: one the TCP build accepts whose TCP-only bytes 52..57 (ack, window) are 0.
VPC_TB_FN bool udp_build_hdr_ok(const uint32_t (&t)[16]) {
    return tcp_build_hdr_ok(t) && t[13] == 0 && (t[14] & 0xffffu) == 0;
}

// Header bytes of a frame of an accepted template: l2_len + (20 | 40) + 8
VPC_TB_FN uint32_t udp_build_header_len(const uint32_t (&t)[16]) { return tb_header_len(t, kUdpHeader); }

// L of an accepted template and a payload of data_len bytes that udp_build_fits accepts
VPC_TB_FN uint32_t udp_build_frame_len(const uint32_t (&t)[16], uint32_t data_len) {
    return udp_build_header_len(t) + data_len;
}

// Whether the datagram of an accepted template fits: 28 + data_len (IPv4 totalLength) or 8 + data_len
// (IPv6 payloadLength, and the UDP length field) within 16 bits, the chunk's room, both arenas;
// nothing wraps for any 32-bit data_len.
VPC_TB_FN bool udp_build_fits(const uint32_t (&t)[16], uint64_t frame_off, uint64_t data_off, uint32_t frame_cap,
                              uint32_t data_len, uint64_t dst_len, uint64_t src_len) {
    return tb_fits(t, kUdpHeader, frame_off, data_off, frame_cap, data_len, dst_len, src_len);
}

// The header's words, sums left 0 (tcp_build.h TcpBuildWords' layout, with 2 UDP words)
struct UdpBuildWords {
    uint32_t eth[4];
    uint32_t ip[10];
    uint32_t udp[2];
};

VPC_TB_FN void udp_build_words(const uint32_t (&t)[16], uint32_t data_len, UdpBuildWords& w) {
    tb_eth_ip_words(t, 17u, kUdpHeader, data_len, w.eth, w.ip);
    // UdpPacket.buildCommonPart (UdpPacket.java:68-94): ports | length 8 + data_len, sum 0
    w.udp[0] = t[12];
    w.udp[1] = tb_bswap16(kUdpHeader + data_len);
}

// The one's complement sum, in the words' own (little-endian) domain, of what the UDP sum covers
// besides the payload: pseudo-header addresses, protocol 17, the length, the UDP header with its sum
// 0.  Not folded.
VPC_TB_FN uint64_t udp_build_l4_header_sum(const uint32_t (&t)[16], const UdpBuildWords& w, uint32_t data_len) {
    return tb_add_pseudo_sum((uint64_t)w.udp[0] + w.udp[1], t, 17u, kUdpHeader, data_len);
}

VPC_TB_FN uint64_t udp_build_ip_header_sum(const UdpBuildWords& w) {
    return (uint64_t)w.ip[0] + w.ip[1] + w.ip[2] + w.ip[3] + w.ip[4];
}

// The UDP field as it lies in the words, from the folded little-endian sum of everything it covers:
// its complement, and 0xffff for a computed 0 (UdpPacket.buildIPv4UdpPacket / buildIPv6UdpPacket,
// UdpPacket.java:96-124; 0xffff reads the same in either byte order)
VPC_TB_FN uint32_t udp_build_l4_field(uint32_t folded) {
    const uint32_t f = 0xffffu - folded;
    return f ? f : 0xffffu;
}

// Put the sums in: the 16 bits as they lie in the words
VPC_TB_FN void udp_build_set_sums(UdpBuildWords& w, bool v4, uint32_t ip_field, uint32_t l4_field) {
    if (v4) w.ip[2] |= ip_field << 16;
    w.udp[1] |= l4_field << 16;
}

#ifndef __HIP_DEVICE_COMPILE__
// Host: the header bytes (sums as the words hold them) as they lie in the frame; returns their count
inline uint32_t udp_build_header_bytes(const UdpBuildWords& w, const uint32_t (&t)[16], uint8_t* out) {
    return tb_header_bytes(w.eth, w.ip, w.udp, kUdpHeader, t, out);
}
#endif

}  // namespace vpcsum
