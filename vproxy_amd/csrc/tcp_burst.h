// tcp_burst.h -- the rules of the TCP send bursts that are not HIP (vpcsum_tcp_build_bursts_async,
// include/vpcsum.h): which burst a frame of the table belongs to, the record of tcp_build.h it is
// built from, and the refusals of a whole burst.  Plain C++, shared by the kernel (tcp_build.hip
// k_tcp_build_bursts), the host entry (api.cpp) and a stand-alone test (tests/cpp/tcp_burst_test.cpp).
//
// The search is 9-ary: a step probes 8 pivots of the open interval and keeps the piece between the
// last pivot whose burst starts at or before the frame and the pivot after it.  On the device the 8
// lanes of a frame's team probe one pivot each and agree by a ballot; the host walks the same pivots
// in a loop.  Nothing here trusts what the search returns: tcp_burst_covers is checked on the record
// that was found, so an unsorted table costs a frame its burst, never a bound.
#pragma once
#include <stdint.h>

#include "tcp_build.h"

namespace vpcsum {

static_assert(sizeof(vpcsum_tcpburst_t) == 32, "vpcsum.h: burst record 32 B");

// A burst record's fields, from its 8 little-endian dwords
struct TcpBurst {
    uint64_t data_off;
    uint32_t data_len, seq, hdr, first, mss, flags, rsv, count;
};

VPC_TB_FN TcpBurst tcp_burst_unpack(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6,
                                    uint32_t w7) {
    TcpBurst b;
    b.data_off = ((uint64_t)w1 << 32) | w0;
    b.data_len = w2;
    b.seq = w3;
    b.hdr = w4;
    b.first = w5;
    b.mss = w6 & 0xffffu;
    b.flags = (w6 >> 16) & 0xffu;
    b.rsv = w6 >> 24;
    b.count = w7;
    return b;
}

// ---- the search: how many bursts start at or before frame j, given a non-decreasing `first` ----
// The answer lies in [lo, hi], from [0, n_bursts]; the frame's burst is the answer - 1.
constexpr uint32_t kTcpBurstPivots = 8;

// Pivot i (0..7) of [lo, hi), lo < hi: inside it, non-decreasing in i
VPC_TB_FN uint32_t tcp_burst_pivot(uint32_t lo, uint32_t hi, uint32_t i) {
    return lo + (uint32_t)(((uint64_t)(hi - lo) * (i + 1u)) / (kTcpBurstPivots + 1u));
}

// One step.  bits: bit i set when first[pivot i] <= j.  The leading run of set bits is what counts
// (a sorted table sets no other): m of them put the answer past pivot m - 1 and at or before pivot
// m.  The interval shrinks at every step, whatever the bits.
VPC_TB_FN void tcp_burst_narrow(uint32_t& lo, uint32_t& hi, uint32_t bits) {
    const uint32_t m = (uint32_t)__builtin_ctz(~bits | (1u << kTcpBurstPivots));
    const uint32_t below = m ? tcp_burst_pivot(lo, hi, m - 1u) + 1u : lo;
    const uint32_t above = m < kTcpBurstPivots ? tcp_burst_pivot(lo, hi, m) : hi;
    lo = below;
    hi = above;
}

// ---- the found record against the frame ----
// Frame j is piece k = j - first of the burst: only then is anything built from it
VPC_TB_FN bool tcp_burst_covers(const TcpBurst& b, uint32_t j) { return j >= b.first && j - b.first < b.count; }

// max(1, ceil(data_len / mss)), mss > 0 or data_len == 0
VPC_TB_FN uint32_t tcp_burst_count(uint32_t data_len, uint32_t mss) { return data_len ? (data_len - 1u) / mss + 1u : 1u; }

// The payload of the burst's longest frame
VPC_TB_FN uint32_t tcp_burst_longest(const TcpBurst& b) { return b.data_len < b.mss ? b.data_len : b.mss; }

// The whole-burst refusals that need the (accepted) template's words; hdr < n_hdr, the flags and
// rsv are tcp_build_seg_ok's, the template's own tcp_build_hdr_ok's.
VPC_TB_FN bool tcp_burst_ok(const uint32_t (&t)[16], const TcpBurst& b, uint32_t frame_cap, uint64_t src_len) {
    if (b.data_len && !b.mss) return false;
    if (b.count != tcp_burst_count(b.data_len, b.mss)) return false;
    const uint32_t longest = b.data_len ? tcp_burst_longest(b) : 0u;
    const uint32_t l3_words = tb_l3_ver(t) == 4 ? 40u : 20u;
    if (l3_words + longest > 65535u) return false;
    if (tcp_build_frame_len(t, longest) > frame_cap) return false;
    if (b.data_off > src_len || (uint64_t)b.data_len > src_len - b.data_off) return false;
    return true;
}

// Piece k of a burst (k < count; of a refused burst the values are not used): where its payload
// lies, its sequence number and its length.  k * mss < data_len, so nothing but seq wraps.
struct TcpBurstPiece {
    uint64_t data_off;
    uint32_t seq, data_len;
};
VPC_TB_FN TcpBurstPiece tcp_burst_piece(const TcpBurst& b, uint32_t k) {
    const uint32_t skip = b.data_len ? k * b.mss : 0u;
    const uint32_t left = b.data_len - skip;
    TcpBurstPiece p;
    p.data_off = b.data_off + skip;
    p.seq = b.seq + skip;
    p.data_len = left < b.mss ? left : (b.data_len ? b.mss : 0u);
    return p;
}

#ifndef __HIP_DEVICE_COMPILE__
inline TcpBurst tcp_burst_fields(const vpcsum_tcpburst_t& r) {
    TcpBurst b;
    b.data_off = r.data_off; b.data_len = r.data_len; b.seq = r.seq; b.hdr = r.hdr; b.first = r.first;
    b.mss = r.mss; b.flags = r.flags; b.rsv = r.rsv; b.count = r.count;
    return b;
}

// Host: the search as the team runs it, the 8 probes of a step one after another.  Returns how many
// bursts start at or before j by a sorted table's reading (0: none); every index it reads is below
// n_bursts.
inline uint32_t tcp_burst_find(const vpcsum_tcpburst_t* bursts, uint32_t n_bursts, uint32_t j) {
    uint32_t lo = 0, hi = n_bursts;
    while (lo < hi) {
        uint32_t bits = 0;
        for (uint32_t i = 0; i < kTcpBurstPivots; ++i)
            if (bursts[tcp_burst_pivot(lo, hi, i)].first <= j) bits |= 1u << i;
        tcp_burst_narrow(lo, hi, bits);
    }
    return lo;
}

// Host: frame j of a call as the kernel plans it.  False: refused; else *seg is the record of
// vpcsum_tcp_build_async it is built from, inside the destination and inside its burst's source range.
inline bool tcp_burst_frame(const vpcsum_tcphdr_t* hdrs, uint32_t n_hdr, const vpcsum_tcpburst_t* bursts, uint32_t n_bursts,
                            uint64_t frame_off, uint32_t j, uint32_t frame_cap, uint64_t dst_len, uint64_t src_len,
                            vpcsum_tcpseg_t* seg, uint32_t* burst_index = nullptr) {
    const uint32_t c = tcp_burst_find(bursts, n_bursts, j);
    if (!c) return false;
    const TcpBurst b = tcp_burst_fields(bursts[c - 1u]);
    if (burst_index) *burst_index = c - 1u;
    if (!tcp_burst_covers(b, j) || !tcp_build_seg_ok(b.hdr, n_hdr, b.flags, b.rsv)) return false;
    uint32_t t[16];
    tcp_build_template_words(hdrs[b.hdr], t);
    if (!tcp_build_hdr_ok(t) || !tcp_burst_ok(t, b, frame_cap, src_len)) return false;
    const TcpBurstPiece p = tcp_burst_piece(b, j - b.first);
    if (!tcp_build_fits(t, frame_off, p.data_off, frame_cap, p.data_len, dst_len, src_len)) return false;
    seg->frame_off = frame_off;
    seg->data_off = p.data_off;
    seg->seq = p.seq;
    seg->hdr = b.hdr;
    seg->frame_cap = frame_cap;
    seg->data_len = (uint16_t)p.data_len;
    seg->flags = (uint8_t)b.flags;
    seg->rsv = 0;
    return true;
}
#endif

// Host: tcp_build_payload_span / tcp_build_rebase_payloads for bursts (vpcsum_ctx_build_tcp_bursts, a
// pageable source): the span covers every non-empty burst payload that lies inside the source, by
// tcp_burst_ok's source rule; a payload outside stays outside (UINT64_MAX: refused by the kernel), an
// empty one reads nothing (0), every other one is rebased to lo.
inline bool tcp_burst_payload_span(const vpcsum_tcpburst_t* burst, uint32_t n, uint64_t src_len, uint64_t capacity,
                                   TcpPayloadSpan* sp) {
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const vpcsum_tcpburst_t& r = burst[i];
        if (!r.data_len || r.data_off > src_len || r.data_len > src_len - r.data_off) continue;
        if (r.data_off < lo) lo = r.data_off;
        if (r.data_off + r.data_len > hi) hi = r.data_off + r.data_len;
    }
    *sp = hi > lo ? TcpPayloadSpan{lo, hi - lo} : TcpPayloadSpan{0, 0};
    return sp->len <= capacity;
}

inline void tcp_burst_rebase_payloads(vpcsum_tcpburst_t* burst, uint32_t n, uint64_t src_len, uint64_t lo) {
    for (uint32_t i = 0; i < n; ++i) {
        vpcsum_tcpburst_t& r = burst[i];
        if (r.data_off > src_len || r.data_len > src_len - r.data_off) r.data_off = UINT64_MAX;
        else r.data_off = r.data_len ? r.data_off - lo : 0;
    }
}

}  // namespace vpcsum
