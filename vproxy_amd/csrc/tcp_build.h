// tcp_build.h -- the rules of the TCP segment build that are not HIP (vpcsum_tcp_build_async,
// include/vpcsum.h): which records are refused, the frame length L, and the header bytes without
// their two sums, from a template (vpcsum_tcphdr_t) and a record (vpcsum_tcpseg_t).  Plain C++,
// shared by the kernel (tcp_build.hip), the host entry (api.cpp) and a stand-alone test
// (tests/cpp/tcp_build_test.cpp).
//
// The header is kept as little-endian dwords of its wire bytes, piece by piece -- Ethernet (14 B in
// 4 words), IP (5 or 10 words), TCP (5 words) -- so that the kernel holds every word in a register
// under a compile-time index and the sums are plain dword adds.  The template travels the same way:
// its 64 bytes as 16 little-endian dwords (a host caller memcpy's the struct into them).
//   t[0..2]  eth_dst, eth_src          t[3]      l2_len | l3_ver << 8 | tos << 16 | ttl << 24
//   t[4..7]  src                       t[8..11]  dst
//   t[12]    sport | dport << 16       t[13]     ack
//   t[14]    window | ident << 16      t[15]     frag | rsv << 16
#pragma once
#include <stdint.h>

#include "vpcsum.h"

#ifdef __HIPCC__
#define VPC_TB_FN __host__ __device__ __forceinline__
#else
#define VPC_TB_FN inline
#endif

namespace vpcsum {

static_assert(sizeof(vpcsum_tcphdr_t) == 64 && sizeof(vpcsum_tcpseg_t) == 32, "vpcsum.h: template 64 B, record 32 B");

constexpr uint32_t kTcpBuildMaxHeader = 74;   // 14 + 40 + 20

VPC_TB_FN uint32_t tb_bswap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }
VPC_TB_FN uint32_t tb_bswap32(uint32_t v) {
    return (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
}

VPC_TB_FN uint32_t tb_l2_len(const uint32_t (&t)[16]) { return t[3] & 0xffu; }
VPC_TB_FN uint32_t tb_l3_ver(const uint32_t (&t)[16]) { return (t[3] >> 8) & 0xffu; }

// The record's own words: flags within TcpPacket.setFlags' 6 bits, rsv 0, a template that exists.
// Checked before the template is read.
VPC_TB_FN bool tcp_build_seg_ok(uint32_t hdr, uint32_t n_hdr, uint32_t flags, uint32_t rsv) {
    return hdr < n_hdr && (flags & ~0x3fu) == 0 && rsv == 0;
}

// The template: IPv4 / IPv6, an Ethernet header or none, rsv 0.
VPC_TB_FN bool tcp_build_hdr_ok(const uint32_t (&t)[16]) {
    const uint32_t l2 = tb_l2_len(t), ver = tb_l3_ver(t);
    return (ver == 4 || ver == 6) && (l2 == 0 || l2 == 14) && (t[15] >> 16) == 0;
}

// Header bytes of a frame of an accepted template with an L4 header of l4_hdr bytes (TCP 20, UDP 8):
// l2_len + (20 | 40) + l4_hdr
VPC_TB_FN uint32_t tb_header_len(const uint32_t (&t)[16], uint32_t l4_hdr) {
    return tb_l2_len(t) + (tb_l3_ver(t) == 4 ? 20u : 40u) + l4_hdr;
}

// Header bytes of a frame of an accepted template: l2_len + (20 | 40) + 20
VPC_TB_FN uint32_t tcp_build_header_len(const uint32_t (&t)[16]) { return tb_header_len(t, 20u); }

// L of an accepted template and a payload of data_len bytes
VPC_TB_FN uint32_t tcp_build_frame_len(const uint32_t (&t)[16], uint32_t data_len) {
    return tcp_build_header_len(t) + data_len;
}

// Whether the frame of an accepted template and an L4 header of l4_hdr bytes fits: its length field
// (Java would truncate the value silently; the build refuses), the chunk's room, and both arenas,
// without wrapping -- data_len may be any 32-bit value.
VPC_TB_FN bool tb_fits(const uint32_t (&t)[16], uint32_t l4_hdr, uint64_t frame_off, uint64_t data_off, uint32_t frame_cap,
                       uint32_t data_len, uint64_t dst_len, uint64_t src_len) {
    const uint32_t counted = tb_l3_ver(t) == 4 ? 20u + l4_hdr : l4_hdr;   // what the length field counts besides the payload
    if (data_len > 65535u || counted + data_len > 65535u) return false;
    const uint32_t L = tb_header_len(t, l4_hdr) + data_len;
    if (L > frame_cap) return false;
    if (frame_off > dst_len || (uint64_t)L > dst_len - frame_off) return false;
    if (data_off > src_len || (uint64_t)data_len > src_len - data_off) return false;
    return true;
}

VPC_TB_FN bool tcp_build_fits(const uint32_t (&t)[16], uint64_t frame_off, uint64_t data_off, uint32_t frame_cap,
                              uint32_t data_len, uint64_t dst_len, uint64_t src_len) {
    return tb_fits(t, 20u, frame_off, data_off, frame_cap, data_len, dst_len, src_len);
}

// The header's words, sums left 0.  eth[3]: the EtherType in its low 16 bits.  ip: 5 words (IPv4) or
// 10 (IPv6; an IPv4 header leaves ip[5..9] 0).
struct TcpBuildWords {
    uint32_t eth[4];
    uint32_t ip[10];
    uint32_t tcp[5];
};

// The Ethernet and IP words of a template whose L4 part is protocol `proto` with a header of l4_hdr
// bytes and data_len payload bytes (lengths tb_fits has accepted)
VPC_TB_FN void tb_eth_ip_words(const uint32_t (&t)[16], uint32_t proto, uint32_t l4_hdr, uint32_t data_len, uint32_t (&eth)[4],
                               uint32_t (&ip)[10]) {
    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t tos = (t[3] >> 16) & 0xffu, ttl = t[3] >> 24;
    // Ethernet: Fastpath.remote, Fastpath.local, 0x0800 / 0x86dd (Fastpath.java:39-43)
    eth[0] = t[0];
    eth[1] = t[1];
    eth[2] = t[2];
    eth[3] = v4 ? 0x0008u : 0xdd86u;
    if (v4) {
        // Ipv4Packet.genHeaderWithChecksumUnfilled (:279-294), IHL 5: 45 tos totalLength | ident frag |
        // ttl protocol sum | src | dst
        ip[0] = 0x45u | (tos << 8) | (tb_bswap16(20u + l4_hdr + data_len) << 16);
        ip[1] = (t[14] >> 16) | (t[15] << 16);
        ip[2] = ttl | (proto << 8);
        ip[3] = t[4];
        ip[4] = t[8];
        ip[5] = ip[6] = ip[7] = ip[8] = ip[9] = 0;
    } else {
        // Ipv6Packet.buildPacket (:185-190): 6 | traffic class | flow label 0 | payloadLength next header hop limit
        ip[0] = (0x60u | (tos >> 4)) | (((tos << 4) & 0xffu) << 8);
        ip[1] = tb_bswap16(l4_hdr + data_len) | (proto << 16) | (ttl << 24);
        ip[2] = t[4]; ip[3] = t[5]; ip[4] = t[6]; ip[5] = t[7];
        ip[6] = t[8]; ip[7] = t[9]; ip[8] = t[10]; ip[9] = t[11];
    }
}

// s plus the one's complement sum, in the words' own (little-endian) domain, of the pseudo-header:
// the addresses, the protocol and the L4 length.  Not folded.
VPC_TB_FN uint64_t tb_add_pseudo_sum(uint64_t s, const uint32_t (&t)[16], uint32_t proto, uint32_t l4_hdr, uint32_t data_len) {
    s += (uint64_t)t[4] + t[8];
    if (tb_l3_ver(t) != 4) s += (uint64_t)t[5] + t[6] + t[7] + t[9] + t[10] + t[11];
    return s + (proto << 8) + tb_bswap16(l4_hdr + data_len);
}

VPC_TB_FN void tcp_build_words(const uint32_t (&t)[16], uint32_t seq, uint32_t data_len, uint32_t flags, TcpBuildWords& w) {
    tb_eth_ip_words(t, 6u, 20u, data_len, w.eth, w.ip);
    // TcpPacket.buildCommonPart (:394-452), no options: ports | seq | ack | 50 flags window | sum urgent 0
    w.tcp[0] = t[12];
    w.tcp[1] = tb_bswap32(seq);
    w.tcp[2] = t[13];
    w.tcp[3] = 0x50u | (flags << 8) | (t[14] << 16);
    w.tcp[4] = 0;
}

// The one's complement sum, in the words' own (little-endian) domain, of what the TCP sum covers
// besides the payload: pseudo-header addresses, protocol 6, the segment length, the TCP header with
// its sum 0.  Not folded.
VPC_TB_FN uint64_t tcp_build_l4_header_sum(const uint32_t (&t)[16], const TcpBuildWords& w, uint32_t data_len) {
    const uint64_t s = (uint64_t)w.tcp[0] + w.tcp[1] + w.tcp[2] + w.tcp[3] + w.tcp[4];
    return tb_add_pseudo_sum(s, t, 6u, 20u, data_len);
}

// The same for the IPv4 header (5 words, sum 0)
VPC_TB_FN uint64_t tcp_build_ip_header_sum(const TcpBuildWords& w) {
    return (uint64_t)w.ip[0] + w.ip[1] + w.ip[2] + w.ip[3] + w.ip[4];
}

// A sum of little-endian words folded end-around to 16 bits (0 only for 0), as device_common.h fold64
VPC_TB_FN uint32_t tb_fold64(uint64_t x) {
    uint64_t v = (x & 0xffffffffull) + (x >> 32);
    v = (v & 0xffff) + (v >> 16);
    v = (v & 0xffff) + (v >> 16);
    v = (v & 0xffff) + (v >> 16);
    return (uint32_t)v;
}

// Put the sums in.  ip_field / l4_field: the 16 bits as they lie in the words (0xffff - the folded
// little-endian sum); the Java ints (ByteArray.int16 of the fields) are their byte swaps.
VPC_TB_FN void tcp_build_set_sums(TcpBuildWords& w, bool v4, uint32_t ip_field, uint32_t l4_field) {
    if (v4) w.ip[2] |= ip_field << 16;
    w.tcp[4] |= l4_field;
}

#ifndef __HIP_DEVICE_COMPILE__
// Host: the template's dwords, and the header bytes (sums 0) of a template and a record as they
// lie in the frame; returns their count (tcp_build_header_len).
inline void tcp_build_template_words(const vpcsum_tcphdr_t& h, uint32_t (&t)[16]) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(&h);
    for (int i = 0; i < 16; ++i)
        t[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}

inline uint32_t tb_header_bytes(const uint32_t* eth, const uint32_t* ip, const uint32_t* l4, uint32_t l4_hdr,
                               const uint32_t (&t)[16], uint8_t* out) {
    uint32_t n = 0;
    auto put = [&](const uint32_t* words, uint32_t bytes) {
        for (uint32_t i = 0; i < bytes; ++i) out[n++] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
    };
    if (tb_l2_len(t) == 14) put(eth, 14);
    put(ip, tb_l3_ver(t) == 4 ? 20 : 40);
    put(l4, l4_hdr);
    return n;
}

inline uint32_t tcp_build_header_bytes(const TcpBuildWords& w, const uint32_t (&t)[16], uint8_t* out) {
    return tb_header_bytes(w.eth, w.ip, w.tcp, 20, t, out);
}
#endif

// Host: the payloads of a batch whose source is staged (vpcsum_ctx_build_tcp_frames, a pageable
// source).  The span [lo, lo + len) covers every non-empty payload that lies inside the source, by
// tcp_build_fits' source rule (nothing wraps: data_off and src_len - data_off are compared, never
// data_off + data_len with an unchecked data_off); len 0: there is none.  False: the span is longer
// than `capacity`, the staging's room.
struct TcpPayloadSpan { uint64_t lo, len; };
template <class Rec>   // vpcsum_tcpseg_t, or another record with data_off / data_len (vpcsum_udpdg_t)
inline bool tcp_build_payload_span(const Rec* seg, uint32_t n, uint64_t src_len, uint64_t capacity,
                                   TcpPayloadSpan* sp) {
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const Rec& r = seg[i];
        if (!r.data_len || r.data_off > src_len || r.data_len > src_len - r.data_off) continue;
        if (r.data_off < lo) lo = r.data_off;
        if (r.data_off + r.data_len > hi) hi = r.data_off + r.data_len;
    }
    *sp = hi > lo ? TcpPayloadSpan{lo, hi - lo} : TcpPayloadSpan{0, 0};
    return sp->len <= capacity;
}

// The records of such a batch, in the library's copy, name the staged span instead of the source: a
// payload outside the source stays outside (UINT64_MAX: refused by the kernel), an empty one reads
// nothing (0), every other one is rebased to lo.
template <class Rec>
inline void tcp_build_rebase_payloads(Rec* seg, uint32_t n, uint64_t src_len, uint64_t lo) {
    for (uint32_t i = 0; i < n; ++i) {
        Rec& r = seg[i];
        if (r.data_off > src_len || r.data_len > src_len - r.data_off) r.data_off = UINT64_MAX;
        else r.data_off = r.data_len ? r.data_off - lo : 0;
    }
}

}  // namespace vpcsum
