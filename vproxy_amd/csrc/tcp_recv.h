// tcp_recv.h -- the rules of the TCP receive that are not HIP (vpcsum_tcp_recv_async and
// vpcsum_tcp_digest_async, include/vpcsum.h): which records are refused, the header length hlen and
// the payload length data_len of a segment, and how many bytes a record stores.  Plain C++, shared by
// the kernels (tcp_recv.hip), the host entry (api.cpp) and a stand-alone test
// (tests/cpp/tcp_recv_test.cpp).
//
// The rule runs in three steps, so that a refused record reads as little as the step that refuses
// it needs: the descriptor and the record's own words (nothing of the arena), then the TCP header's
// byte 12 (the data offset), then the record against the payload and the destination.
#pragma once
#include <stdint.h>

#include "vpcsum.h"

#ifdef __HIPCC__
#define VPC_TR_FN __host__ __device__ __forceinline__
#else
#define VPC_TR_FN inline
#endif

namespace vpcsum {

static_assert(sizeof(vpcsum_tcprx_t) == 16 && sizeof(vpcsum_tcpinfo_t) == 16, "vpcsum.h: record 16 B, digest 16 B");

// Step 1, the descriptor: TCP with F_L4 alone (or with F_IP on IPv4) whose packet lies in the arena
// and whose L4 offset is one vpcsum_compute_async takes (IPv4: 20..60 in steps of 4 -- the pseudo
// header is read at bytes 12..19 --, IPv6: at least 40), with a segment of at least 20 bytes.
// Nothing wraps: l3_off and arena_len - l3_off are compared.
// (l4_recv_desc_ok: the same rule for protocol `proto` with a segment of at least min_seg bytes; the
// UDP receive, udp_recv.h, asks for 17 and 8.)
VPC_TR_FN bool l4_recv_desc_ok(uint32_t proto, uint32_t min_seg, uint64_t l3_off, uint32_t l3_len, uint32_t l4_off,
                               uint32_t l3_ver, uint32_t l4_proto, uint32_t flags, uint64_t arena_len) {
    if (l4_proto != proto) return false;
    if (l3_ver != 4u && l3_ver != 6u) return false;
    if (!(flags & VPCSUM_F_L4) || (flags & (VPCSUM_F_L4P | VPCSUM_F_RAW | VPCSUM_F_PRE))) return false;
    if ((flags & VPCSUM_F_IP) && l3_ver != 4u) return false;
    if (l4_off > l3_len) return false;
    if (l3_ver == 4u ? (l4_off < 20u || (l4_off & 3u)) : l4_off < 40u) return false;
    if (l3_off > arena_len || (uint64_t)l3_len > arena_len - l3_off) return false;
    return l3_len - l4_off >= min_seg;
}
VPC_TR_FN bool tcp_recv_desc_ok(uint64_t l3_off, uint32_t l3_len, uint32_t l4_off, uint32_t l3_ver, uint32_t l4_proto,
                                uint32_t flags, uint64_t arena_len) {
    return l4_recv_desc_ok(6u, 20u, l3_off, l3_len, l4_off, l3_ver, l4_proto, flags, arena_len);
}

// The record's own words: no operation but STORE, rsv 0.
VPC_TR_FN bool tcp_recv_ops_ok(uint32_t ops, uint32_t rsv) { return (ops & ~VPCSUM_TCPRX_STORE) == 0 && rsv == 0; }

// Step 2, the header: byte 12 of a segment of seg_len >= 20 bytes (TcpPacket.from, TcpPacket.java:
// 223-240: data offset * 4, at least 20 and no longer than the segment).
VPC_TR_FN bool tcp_recv_hdr_ok(uint32_t seg_len, uint32_t byte12, uint32_t* hlen, uint32_t* data_len) {
    const uint32_t h = ((byte12 >> 4) & 0xfu) * 4u;
    if (h < 20u || h > seg_len) return false;
    *hlen = h;
    *data_len = seg_len - h;
    return true;
}

// Step 3, the record against the payload and the destination: the bytes it stores (0 without STORE),
// refused when skip passes the payload, the room at dst_off is short or the range leaves the
// destination (no wrap).
VPC_TR_FN bool tcp_recv_store_ok(uint32_t data_len, uint32_t skip, uint32_t ops, uint64_t dst_off, uint32_t dst_cap,
                                 uint64_t dst_len, uint32_t* stored) {
    if (skip > data_len) return false;
    *stored = 0;
    if (!(ops & VPCSUM_TCPRX_STORE)) return true;
    const uint32_t st = data_len - skip;
    if (st > dst_cap) return false;
    if (dst_off > dst_len || (uint64_t)st > dst_len - dst_off) return false;
    *stored = st;
    return true;
}

#ifndef __HIP_DEVICE_COMPILE__
// Host: the whole rule on a descriptor, a record and the segment's byte 12 (read through `byte12_at`
// only when step 1 passed).  What the kernel decides, for the stand-alone test and host callers.
struct TcpRecvPlan { uint32_t hlen, data_len, stored; };
template <class Byte12>
inline bool tcp_recv_plan(const vpcsum_desc_t& d, const vpcsum_tcprx_t& r, uint64_t arena_len, uint64_t dst_len,
                          Byte12 byte12_at, TcpRecvPlan* p) {
    *p = TcpRecvPlan{0, 0, 0};
    if (!tcp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len)) return false;
    if (!tcp_recv_ops_ok(r.ops, r.rsv)) return false;
    uint32_t hlen = 0, data_len = 0, stored = 0;
    if (!tcp_recv_hdr_ok((uint32_t)d.l3_len - d.l4_off, byte12_at(d.l3_off + d.l4_off + 12u), &hlen, &data_len)) return false;
    if (!tcp_recv_store_ok(data_len, r.skip, r.ops, r.dst_off, r.dst_cap, dst_len, &stored)) return false;
    *p = TcpRecvPlan{hlen, data_len, stored};
    return true;
}
#endif

}  // namespace vpcsum
