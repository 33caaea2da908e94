// batch_plan.h -- the host arithmetic of the context's batch path (api.cpp): which bytes of the
// caller's arena a batch touches and how they are laid out in the pinned staging.  Pure functions of
// host memory, no HIP: tests/cpp/batch_plan_test.cpp runs them under the sanitizers with plain g++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "vpcsum.h"

namespace vpcsum {

// The kernels' bounds rule: a descriptor outside the arena is flagged S_BAD_DESC there, and never
// read on the host.
inline bool desc_in_arena(const vpcsum_desc_t& d, uint64_t arena_len) {
    return d.l3_off <= arena_len && d.l3_len <= arena_len - d.l3_off;
}

// Offset of the L4 checksum field in its header, -1: the protocol has none (the host copy of
// device_common.h l4_field).
inline int l4_field_host(int proto) { return proto == 6 ? 16 : proto == 17 ? 6 : (proto == 1 || proto == 58) ? 2 : -1; }

// Byte span [lo, hi) the in-arena descriptors touch, lo rounded down to 16 (so device alignment ==
// host alignment), and `used`, their bytes plus 16 each (the sparse-batch test of a staged submit).
// No descriptor in the arena: {0, 0, 0}.
struct BatchSpan {
    uint64_t lo, hi, used;
};
inline BatchSpan batch_span(const vpcsum_desc_t* desc, uint32_t n, uint64_t arena_len) {
    BatchSpan s = {UINT64_MAX, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        const vpcsum_desc_t& d = desc[i];
        if (!desc_in_arena(d, arena_len)) continue;
        s.lo = std::min(s.lo, d.l3_off);
        s.hi = std::max(s.hi, d.l3_off + d.l3_len);
        s.used += d.l3_len + 16;
    }
    if (s.lo == UINT64_MAX) return {0, 0, 0};
    s.lo &= ~(uint64_t)15;
    return s;
}

struct TakeWholePacket {
    uint32_t operator()(uint32_t, const vpcsum_desc_t& d) const { return d.l3_len; }
};

// Gather each packet's 16-B blocks into `stage`: out_desc[i] is in[i] with l3_off rebased to the
// staging (same offset mod 16) and l3_len = take(i, in[i]), the bytes of packet i to carry (at most
// its l3_len); a descriptor outside the arena gets l3_off UINT64_MAX and is not read.  Returns the
// staged bytes (a multiple of 16), or -1 when they would exceed `capacity`.
template <class Take = TakeWholePacket>
inline int64_t gather_blocks(const uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* in, uint32_t n,
                             vpcsum_desc_t* out_desc, uint8_t* stage, uint64_t capacity, Take take = Take()) {
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const vpcsum_desc_t& d = in[i];
        out_desc[i] = d;
        if (!desc_in_arena(d, arena_len)) { out_desc[i].l3_off = UINT64_MAX; continue; }
        const uint32_t len = take(i, d);
        out_desc[i].l3_len = (uint16_t)len;
        const uint64_t a0 = d.l3_off & ~(uint64_t)15;
        const uint64_t a1 = std::min<uint64_t>((d.l3_off + len + 15) & ~(uint64_t)15, arena_len);
        if (pos + (a1 - a0) > capacity) return -1;
        memcpy(stage + pos, h_arena + a0, a1 - a0);
        out_desc[i].l3_off = pos + (d.l3_off - a0);
        pos += (a1 - a0 + 15) & ~(uint64_t)15;
    }
    return (int64_t)pos;
}

// Bytes of a NAT'd packet the rewrite can change: the L3 header through the L4 checksum field.  A
// staged NAT batch copies that much of each packet back into the caller's frames.
inline uint32_t nat_header_end(const vpcsum_desc_t& d) {
    const int fld = l4_field_host(d.l4_proto);
    uint32_t end = d.l3_ver == 4 ? 20 : 40;
    if (fld >= 0 && d.l3_len >= d.l4_off + fld + 2) end = std::max<uint32_t>(end, d.l4_off + fld + 2u);
    return std::min<uint32_t>(end, d.l3_len);
}

// The same under VPCSUM_NAT_TCP_REWRITES: a TCP packet with its 20-byte header in the segment can
// also change in its sequence number, flags and options, so its whole TCP header goes back, taken
// at the longest a data offset allows (60 bytes; the bytes past the real header return unchanged).
inline uint32_t nat_tcp_header_end(const vpcsum_desc_t& d) {
    if (d.l4_proto == 6 && d.l3_len >= d.l4_off + 20u)
        return std::max<uint32_t>(nat_header_end(d), std::min<uint32_t>(d.l4_off + 60u, d.l3_len));
    return nat_header_end(d);
}

// The header return of a finished staged NAT batch: what the rewrite can have changed of packet i
// (nat_header_end; `tcp`, under VPCSUM_NAT_TCP_REWRITES: nat_tcp_header_end) goes from the staging at
// stage_desc[i] (gather_blocks' descriptor) into the caller's frame at desc[i]; not if refused (S_BAD_DESC).
inline void return_nat_headers(uint8_t* arena, const vpcsum_desc_t* desc, const uint8_t* stage, const vpcsum_desc_t* stage_desc,
                               const uint8_t* status, uint32_t n, bool tcp) {
    for (uint32_t i = 0; i < n; ++i) {
        if (status[i] & VPCSUM_S_BAD_DESC) continue;
        const vpcsum_desc_t& d = desc[i];
        memcpy(arena + d.l3_off, stage + stage_desc[i].l3_off, tcp ? nat_tcp_header_end(d) : nat_header_end(d));
    }
}

// The placement of a finished staged MODE_WRITE batch: out[i] -- the IP sum in the low half, the L4
// sum in the high half -- into the checksum fields of the caller's frames (big endian, as
// ByteArray.int16).  A packet the kernel refused (S_BAD_DESC) is untouched.
inline void place_checksums(uint8_t* arena, const vpcsum_desc_t* desc, const uint32_t* out, const uint8_t* status, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        const vpcsum_desc_t& d = desc[i];
        if (status[i] & VPCSUM_S_BAD_DESC) continue;
        uint8_t* l3 = arena + d.l3_off;
        const uint32_t w = out[i];
        if (d.flags & VPCSUM_F_IP) { l3[10] = (uint8_t)(w >> 8); l3[11] = (uint8_t)w; }
        if (d.flags & (VPCSUM_F_L4 | VPCSUM_F_L4P)) {
            const int fld = l4_field_host(d.l4_proto);
            if (fld < 0) continue;   // no L4 sum: the kernel refused the descriptor (BAD above)
            l3[d.l4_off + fld] = (uint8_t)(w >> 24);
            l3[d.l4_off + fld + 1] = (uint8_t)(w >> 16);
        }
    }
}

// The mask byte of a pre-image entry (vpcsum_pre_t / vpcsum_pre4_t).
inline uint8_t pre_entry_mask(const void* entry, uint32_t pre_fmt) {
    return ((const uint8_t*)entry)[pre_fmt == VPCSUM_PRE_FMT_PRE ? offsetof(vpcsum_pre_t, mask) : offsetof(vpcsum_pre4_t, mask)];
}

// Bytes of in-arena packet d a staged pre-image batch carries.  An F_PRE packet with an L4 sum to
// update: its header through the checksum field, or through the L4 header that a header-sum entry
// (VPCSUM_PRE_HSUM) covers -- *cut is set, the kernel reads no further -- unless it is UDP with a
// stored 0, which is summed in full.  Any other packet: all of it.  entry: the packet's
// vpcsum_pre_t / vpcsum_pre4_t.
inline uint32_t pre_staged_len(const uint8_t* h_arena, const vpcsum_desc_t& d, const void* entry, uint32_t pre_fmt,
                               bool* cut) {
    *cut = false;
    const int fld = l4_field_host(d.l4_proto);
    if (!(d.flags & VPCSUM_F_PRE) || fld < 0 || (uint32_t)d.l4_off + fld + 2u > d.l3_len) return d.l3_len;
    const uint8_t* f = h_arena + d.l3_off + d.l4_off + fld;
    if (d.l4_proto == 17 && f[0] == 0 && f[1] == 0) return d.l3_len;
    const uint32_t hl =
        (pre_entry_mask(entry, pre_fmt) & VPCSUM_PRE_HSUM) ? ((const uint8_t*)entry)[offsetof(vpcsum_hsum_t, hlen)] : 0u;
    *cut = true;
    const uint32_t take = std::max<uint32_t>(d.l3_ver == 4 ? 20u : 40u, (uint32_t)d.l4_off + std::max<uint32_t>(fld + 2u, hl));
    return std::min<uint32_t>(take, d.l3_len);
}

}  // namespace vpcsum
