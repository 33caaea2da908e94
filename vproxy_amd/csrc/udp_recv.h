// udp_recv.h -- the rules of the UDP receive that are not HIP (vpcsum_udp_recv_async, include/vpcsum.h):
// which records are refused and how many bytes a record stores.  Plain C++, shared by the kernel
// (udp.hip), the host entry (api.cpp) and a stand-alone test (tests/cpp/udp_rules_test.cpp).
//
// Two steps, neither of which reads the arena: the descriptor and the record's own words (tcp_recv.h's
// descriptor rule with protocol 17 and a segment of at least the 8 header bytes), then the record
// against the destination.  The UDP length field is not consulted: the data is segment bytes
// [8, seg_len), as UdpPacket.initPartial takes it (UdpPacket.java:30-38).
#pragma once
#include <stdint.h>

#include "tcp_recv.h"
#include "vpcsum.h"

namespace vpcsum {

static_assert(sizeof(vpcsum_udprx_t) == 16, "vpcsum.h: record 16 B");

// Step 1, the descriptor: UDP with F_L4 alone (or with F_IP on IPv4) whose packet lies in the arena,
// whose L4 offset is one vpcsum_compute_async takes, with a segment of at least 8 bytes.
VPC_TR_FN bool udp_recv_desc_ok(uint64_t l3_off, uint32_t l3_len, uint32_t l4_off, uint32_t l3_ver, uint32_t l4_proto,
                                uint32_t flags, uint64_t arena_len) {
    return l4_recv_desc_ok(17u, 8u, l3_off, l3_len, l4_off, l3_ver, l4_proto, flags, arena_len);
}

// The record's own words: no operation but STORE, rsv (its three bytes as one value) 0.
VPC_TR_FN bool udp_recv_ops_ok(uint32_t ops, uint32_t rsv) { return (ops & ~VPCSUM_UDPRX_STORE) == 0 && rsv == 0; }

// Step 2, the record against the destination: the bytes it stores (0 without STORE), refused when the
// room at dst_off is short or the range leaves the destination (no wrap).  seg_len >= 8.
VPC_TR_FN bool udp_recv_store_ok(uint32_t seg_len, uint32_t ops, uint64_t dst_off, uint32_t dst_cap, uint64_t dst_len,
                                 uint32_t* stored) {
    *stored = 0;
    if (!(ops & VPCSUM_UDPRX_STORE)) return true;
    const uint32_t st = seg_len - 8u;
    if (st > dst_cap) return false;
    if (dst_off > dst_len || (uint64_t)st > dst_len - dst_off) return false;
    *stored = st;
    return true;
}

// The verdict of a datagram whose stored field is `field` and whose sum, recomputed with the field
// taken as 0, is `l4c` before UDP's own rule (host-order values): what vpcsum_compute_async writes
// with VPCSUM_MODE_VERIFY -- a computed 0 counts as 0xffff, a stored 0 is "no checksum" and never OK.
VPC_TR_FN uint32_t udp_recv_l4c(uint32_t l4c) { return l4c ? l4c : 0xffffu; }
VPC_TR_FN uint32_t udp_recv_l4_status(uint32_t field, uint32_t l4c) {
    uint32_t st = 0;
    if (field == udp_recv_l4c(l4c)) st |= VPCSUM_S_L4_OK;
    if (field == 0) st |= VPCSUM_S_UDP_NOCSUM;
    return st;
}

#ifndef __HIP_DEVICE_COMPILE__
// Host: the whole rule on a descriptor and a record.  What the kernel decides, for the stand-alone
// test and host callers.
inline bool udp_recv_plan(const vpcsum_desc_t& d, const vpcsum_udprx_t& r, uint64_t arena_len, uint64_t dst_len,
                          uint32_t* stored) {
    *stored = 0;
    if (!udp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len)) return false;
    if (!udp_recv_ops_ok(r.ops, (uint32_t)r.rsv[0] | ((uint32_t)r.rsv[1] << 8) | ((uint32_t)r.rsv[2] << 16))) return false;
    return udp_recv_store_ok((uint32_t)d.l3_len - d.l4_off, r.ops, r.dst_off, r.dst_cap, dst_len, stored);
}
#endif

}  // namespace vpcsum
