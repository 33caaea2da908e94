// tcp_rewrite.h -- the TCP-header rewrites of a NAT'd packet (VPCSUM_NAT_TCP entries under
// VPCSUM_NAT_TCP_REWRITES): sequence addend, flags, MSS clamp, as the reference's setters do them in
// place.  Plain functions on a byte pointer, no HIP: nat.hip's k_nat_tcp calls them per lane, and
// tests/cpp/tcp_rewrite_test.cpp runs them under the sanitizers with plain g++.
//
//   SwitchUtils.buildSynPacketForProxyProtocol      SwitchUtils.java:461-465  setSeqNum(seq - N)
//   SwitchUtils.buildSynAckPacketForProxyProtocol   :467-473                  setSeqNum(seq - 1), setFlags(SYN|ACK)
//   SwitchUtils.checkAndUpdateMss                   :46-95                    TcpOption.setData (TcpPacket.java:561-569)
//   TcpPacket.setSeqNum / setFlags                  TcpPacket.java:57-63, 90-96: write, then checksumSkipped()
//   TcpPacket.from + TcpOption.check                :241-287, :622-636: the option walk (kernels.hip pe_tcp_from)
#pragma once
#include <stdint.h>

#include "vpcsum.h"

#ifdef __HIPCC__
#define VPC_TCP_FN __host__ __device__ __forceinline__
#else
#define VPC_TCP_FN inline
#endif

namespace vpcsum {

// The TCP part of a vpcsum_nat_t entry (rsv[0..7]), decoded.
struct TcpRw {
    uint32_t ops;       // VPCSUM_TCP_*
    uint32_t flags;     // SET_FLAGS: the new low 6 bits of byte 13
    uint32_t max_mss;   // CLAMP_MSS: the egress port's maxMss
    uint32_t addend;    // SEQ_ADD: added to the sequence number mod 2^32
};

// From the entry's last three little-endian dwords (bytes 36..39: mask, ttl, rsv[0..1]; 40..43:
// rsv[2..5]; 44..47: rsv[6..9]).  Without VPCSUM_NAT_TCP in the mask: no ops.
VPC_TCP_FN TcpRw tcp_rw_decode(uint32_t y, uint32_t z, uint32_t w) {
    TcpRw r;
    r.ops = (y & VPCSUM_NAT_TCP) ? ((y >> 16) & (VPCSUM_TCP_SEQ_ADD | VPCSUM_TCP_SET_FLAGS | VPCSUM_TCP_CLAMP_MSS)) : 0u;
    r.flags = (y >> 24) & 0x3fu;
    r.max_mss = ((z & 0xffu) << 8) | ((z >> 8) & 0xffu);
    r.addend = (((z >> 16) & 0xffu) << 24) | ((z >> 24) << 16) | ((w & 0xffu) << 8) | ((w >> 8) & 0xffu);
    return r;
}
VPC_TCP_FN TcpRw tcp_rw_of_entry(const uint8_t* e) {   // e: the 48 bytes of a vpcsum_nat_t
    const uint32_t y = e[36] | ((uint32_t)e[37] << 8) | ((uint32_t)e[38] << 16) | ((uint32_t)e[39] << 24);
    const uint32_t z = e[40] | ((uint32_t)e[41] << 8) | ((uint32_t)e[42] << 16) | ((uint32_t)e[43] << 24);
    const uint32_t w = e[44] | ((uint32_t)e[45] << 8) | ((uint32_t)e[46] << 16) | ((uint32_t)e[47] << 24);
    return tcp_rw_decode(y, z, w);
}

// The option walk of TcpPacket.from on the header at t, seg bytes of segment (>= 20): -1 when the
// parse fails (data offset past the segment, a length-0 or length-1 option, a length past the data
// offset, MSS length != 4, window-scale length != 3, a kind >= 2 in the last byte), else the offset
// of the first MSS option before any END, 0 when there is none.  Reads t[12] and t[20 .. data
// offset), all inside the segment.
VPC_TCP_FN int tcp_walk_mss(const uint8_t* t, uint32_t seg) {
    const uint32_t doff = (uint32_t)(t[12] >> 4) * 4u;
    if (doff > seg) return -1;
    int mss_at = 0;
    uint32_t off = 20;
    while (off < doff) {   // at most 40 option bytes, each round moves on
        const uint32_t kind = t[off];
        if (kind == 0) break;
        if (kind == 1) { off += 1; continue; }
        if (off + 1 >= doff) return -1;
        const uint32_t ln = t[off + 1];
        if (off + ln > doff || ln < 2) return -1;
        if ((kind == 3 && ln != 3) || (kind == 2 && ln != 4)) return -1;
        if (kind == 2 && !mss_at) mss_at = (int)off;
        off += ln;
    }
    return mss_at;
}

// Overwrites byte k of the TCP header; returns RFC 1624's ~m + m' of its 16-bit word (the word's
// other byte cancels: ~(a:b) + (a:b') = ~(0:b) + (0:b')), so a field at an odd offset -- an MSS
// option after a NOP -- needs no word reads.
VPC_TCP_FN uint32_t tcp_put(uint8_t* t, uint32_t k, uint32_t nb) {
    const int sh = (k & 1) ? 0 : 8;
    const uint32_t m = (uint32_t)t[k] << sh;
    t[k] = (uint8_t)nb;
    return (0xffffu - m) + ((nb & 0xffu) << sh);
}

struct TcpRes {
    uint32_t diff;   // sum of ~m + m' over the bytes written (< 2^20)
    bool dirty;      // Java marked the TCP sum dirty
    bool absent;     // CLAMP_MSS on a SYN whose options parse and hold no MSS option
};

// The setters on the TCP header at t (seg >= 20 bytes of segment, the caller's check): SET_FLAGS,
// SEQ_ADD, then CLAMP_MSS on the flags as they now are.  Writes only t[4..7], t[13] and the two data
// bytes of the first MSS option.
VPC_TCP_FN TcpRes tcp_rewrite(uint8_t* t, uint32_t seg, const TcpRw& r) {
    TcpRes o = {0u, false, false};
    if (r.ops & VPCSUM_TCP_SET_FLAGS) {   // setFlags: byte 12 and the two high bits of 13 stay
        o.diff += tcp_put(t, 13, (t[13] & 0xc0u) | r.flags);
        o.dirty = true;
    }
    if (r.ops & VPCSUM_TCP_SEQ_ADD) {     // setSeqNum: dirty also when the addend is 0
        const uint32_t seq = (((uint32_t)t[4] << 24) | ((uint32_t)t[5] << 16) | ((uint32_t)t[6] << 8) | t[7]) + r.addend;
        o.diff += tcp_put(t, 4, seq >> 24);
        o.diff += tcp_put(t, 5, seq >> 16);
        o.diff += tcp_put(t, 6, seq >> 8);
        o.diff += tcp_put(t, 7, seq);
        o.dirty = true;
    }
    if ((r.ops & VPCSUM_TCP_CLAMP_MSS) && (t[13] & 0x02u)) {
        const int at = tcp_walk_mss(t, seg);
        if (at == 0) {
            o.absent = true;
        } else if (at > 0) {
            const uint32_t mss = ((uint32_t)t[at + 2] << 8) | t[at + 3];
            if (mss > r.max_mss) {
                o.diff += tcp_put(t, (uint32_t)at + 2, r.max_mss >> 8);
                o.diff += tcp_put(t, (uint32_t)at + 3, r.max_mss);
                o.dirty = true;
            }
        }
    }
    return o;
}

// `absent` from the bytes alone, after the rewrite ran (the clamp changes no byte the walk reads):
// strict mode's status pass.
VPC_TCP_FN bool tcp_mss_absent(const uint8_t* t, uint32_t seg, const TcpRw& r) {
    return (r.ops & VPCSUM_TCP_CLAMP_MSS) && (t[13] & 0x02u) && tcp_walk_mss(t, seg) == 0;
}

// RFC 1624 eqn. 3 on the stored TCP sum at t[16..17]: HC' = ~(~HC + diff).  Composes with the
// address / port update already in HC: end-around folds of a non-zero sum stay in 1..0xffff.
VPC_TCP_FN void tcp_sum_update(uint8_t* t, uint32_t diff) {
    const uint32_t hc = ((uint32_t)t[16] << 8) | t[17];
    uint32_t s = (~hc & 0xffffu) + (diff & 0xffffu) + (diff >> 16);
    s = (s & 0xffffu) + (s >> 16);
    s = (s & 0xffffu) + (s >> 16);
    const uint32_t c = ~s & 0xffffu;
    t[16] = (uint8_t)(c >> 8);
    t[17] = (uint8_t)c;
}

// Does the entry's TCP part apply to this packet at all: TCP with the 20-byte header in the segment.
VPC_TCP_FN bool tcp_rw_applies(int proto, int len, int l4o) { return proto == 6 && len - l4o >= 20; }

}  // namespace vpcsum
