// team_move.h -- the payload mover of the TCP kernels (tcp_build.hip k_tcp_build, tcp_recv.hip
// k_tcp_recv) and the piece store (those two and flow.hip k_l2_forward), each held once.
//
// The mover: a team of 8 lanes reads a segment once, adds every byte of it to a one's complement
// accumulator and stores the bytes of a range of it, from the registers that summed them.
//
// Shape: 16 B per lane and step.  The steps follow ONE 16-B grid for the sum and the store, the
// DESTINATION's: segment byte 0 has the destination address v0 -- an integer, dereferenced only
// inside the stored range, so a caller may lay bytes that are summed and not stored (a header, a
// skipped prefix) on addresses that do not exist.  Group g covers the grid's bytes [16 g, 16 g + 16),
// the segment [lo, hi) of them (lo = v0 & 15), the stored range [s_lo, s_hi) inside it; every interior
// group of the stored range leaves in one aligned 16-B store.  emit_group<false> takes the stored
// range to be the segment (the build); emit_group<true> has the sum bound and a second, store-only
// bound (the receive).
//
// Source loads: source and grid are independent modulo 16.  The bytes of group g lie at s0 + 16 g, s0
// of any alignment; they are loaded as the five 4-B aligned dwords W[4g .. 4g+4] around them (one 16-B
// load at 4-B alignment and one dword; the dword only when s0 is not 4-B aligned) and brought into
// place with v_alignbyte by s0 & 3.  Nothing assumes unaligned access.
//
// Edges: a group that is not all segment -- the first and the last -- loads only those of its dwords
// that hold a segment byte (k_lo .. k_hi: no load crosses into a page the segment does not touch, and
// no 16-B load reaches past the last such dword), masks each grid dword to its segment bytes for the
// sum, and stores partial dwords byte by byte (halfwords where both bytes are in range).  No store
// falls outside the stored range.
//
// Sums: 64-bit per lane (65,515 bytes of 0xff are 2,048 dwords per lane), folded once by the caller
// (device_common.h fold64 / fold32).  Summing grid-aligned dwords makes the byte parity one constant
// per segment: the folded sum is byte-swapped against the segment's own 16-bit words when v0 is odd.
//
// The mover also compiles for the host -- the address space, the cache policy and v_alignbyte have
// plain C++ stand-ins there -- so that tests/cpp/team_move_test.cpp runs it under ASan / UBSan.
#pragma once
#include <stdint.h>

#include "device_common.h"

#define VPC_TM_FN __host__ __device__ __forceinline__

namespace vpcsum {

#ifdef __HIP_DEVICE_COMPILE__
#define VPC_TM_LOAD(T, a) __builtin_nontemporal_load((T*)(a))   // read once
VPC_TM_FN uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#else
#define VPC_TM_LOAD(T, a) (*(T*)(a))
VPC_TM_FN uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> ((sh & 3u) * 8u));
}
#endif

// What a lane needs to move the segment's groups.  Byte offsets are relative to `sa` in the source
// and to the grid base `pd` on the destination side, the same number on both.
struct Span {
    uintptr_t sa;        // 4-B aligned: source dword k is at sa + 4 k
    uintptr_t pd;        // 16-B aligned, virtual: group g is at pd + 16 g (only [s_lo, s_hi) of it exists)
    uint32_t sh;         // the source bytes of group g start at sa + 16 g + sh
    uint32_t lo, hi;     // the segment is grid bytes [lo, hi): what is summed
    uint32_t s_lo, s_hi; // the stored range, inside [lo, hi); s_lo == s_hi: nothing is stored
    uint32_t k_lo, k_hi; // the source dwords that hold a segment byte (hi > lo)
};

// The span of the seg_len bytes at `seg` laid on the grid of v0, segment byte 0's (virtual) destination
// address; the bytes from store_from on are stored (0: all of them, seg_len: none).
VPC_TM_FN Span make_span(uintptr_t v0, uintptr_t seg, uint32_t seg_len, uint32_t store_from) {
    Span sp;
    sp.lo = (uint32_t)v0 & 15u;
    sp.hi = sp.lo + seg_len;
    sp.pd = v0 - sp.lo;
    sp.s_lo = sp.lo + store_from;
    sp.s_hi = sp.hi;
    const uintptr_t s0 = seg - sp.lo;
    sp.sh = (uint32_t)s0 & 3u;
    sp.sa = s0 - sp.sh;
    sp.k_lo = (sp.lo + sp.sh) >> 2;
    sp.k_hi = (sp.lo + sp.sh + seg_len - 1u) >> 2;   // read only when seg_len > 0
    return sp;
}

struct Group {
    uint32_t w0, w1, w2, w3, w4;
};

VPC_TM_FN bool group_inner(const Span& sp, uint32_t g) { return g * 16u >= sp.lo && g * 16u + 16u <= sp.hi; }

VPC_TM_FN Group load_group(const Span& sp, uint32_t g) {
    Group r;
    const uintptr_t q = sp.sa + (size_t)g * 16u;
    if (group_inner(sp, g)) {
        // all 16 bytes are segment: W[4g..4g+3] each hold some of them, W[4g+4] too when sh != 0
        const u32x4a4_t v = VPC_TM_LOAD(gu32x4a4_t, q);
        r.w0 = v.x; r.w1 = v.y; r.w2 = v.z; r.w3 = v.w;
        r.w4 = sp.sh ? VPC_TM_LOAD(gu32_t, q + 16) : 0u;
    } else {
        const uint32_t k = g * 4u;
        r.w0 = (k >= sp.k_lo && k <= sp.k_hi) ? VPC_TM_LOAD(gu32_t, q) : 0u;
        r.w1 = (k + 1 >= sp.k_lo && k + 1 <= sp.k_hi) ? VPC_TM_LOAD(gu32_t, q + 4) : 0u;
        r.w2 = (k + 2 >= sp.k_lo && k + 2 <= sp.k_hi) ? VPC_TM_LOAD(gu32_t, q + 8) : 0u;
        r.w3 = (k + 3 >= sp.k_lo && k + 3 <= sp.k_hi) ? VPC_TM_LOAD(gu32_t, q + 12) : 0u;
        r.w4 = (k + 4 >= sp.k_lo && k + 4 <= sp.k_hi) ? VPC_TM_LOAD(gu32_t, q + 16) : 0u;
    }
    return r;
}

// the bytes of dword v that mask m names (not all four, at least one) to the 4-B aligned address a
VPC_TM_FN void store_partial(uintptr_t a, uint32_t v, uint32_t m) {
    if ((m & 0xffffu) == 0xffffu) {
        *(gwu16_t*)a = (uint16_t)v;
    } else {
        if (m & 0xffu) *(gwu8_t*)a = (uint8_t)v;
        if (m & 0xff00u) *(gwu8_t*)(a + 1) = (uint8_t)(v >> 8);
    }
    if ((m >> 16) == 0xffffu) {
        *(gwu16_t*)(a + 2) = (uint16_t)(v >> 16);
    } else {
        if (m & 0xff0000u) *(gwu8_t*)(a + 2) = (uint8_t)(v >> 16);
        if (m & 0xff000000u) *(gwu8_t*)(a + 3) = (uint8_t)(v >> 24);
    }
}

// shift the group into place, add what is segment, store what is in the stored range.  SUB: the
// stored range has bounds of its own; else it is the segment, and [s_lo, s_hi) is not read.
template <bool SUB>
VPC_TM_FN void emit_group(const Span& sp, uint32_t g, const Group& r, uint64_t& acc) {
    uint32_t d0 = alignbyte(r.w1, r.w0, sp.sh);
    uint32_t d1 = alignbyte(r.w2, r.w1, sp.sh);
    uint32_t d2 = alignbyte(r.w3, r.w2, sp.sh);
    uint32_t d3 = alignbyte(r.w4, r.w3, sp.sh);
    const uint32_t rel = g * 16u;
    const uintptr_t p = sp.pd + (size_t)rel;
    const uint32_t s_lo = SUB ? sp.s_lo : sp.lo, s_hi = SUB ? sp.s_hi : sp.hi;
    if (rel >= s_lo && rel + 16u <= s_hi) {
        // all of it is stored, so all of it is segment
        acc += (uint64_t)d0 + d1 + d2 + d3;
        u32x4_t o;
        o.x = d0; o.y = d1; o.z = d2; o.w = d3;
        *(gwu32x4_t*)p = o;
        return;
    }
    if (!SUB || !group_inner(sp, g)) {
        const int lo = (int)sp.lo, hi = (int)sp.hi;
        d0 &= bmask((int)rel, lo, hi);
        d1 &= bmask((int)rel + 4, lo, hi);
        d2 &= bmask((int)rel + 8, lo, hi);
        d3 &= bmask((int)rel + 12, lo, hi);
    }
    acc += (uint64_t)d0 + d1 + d2 + d3;
    if (!SUB || (rel + 16u > s_lo && rel < s_hi)) {
        // the stored range begins or ends in this group
        const int lo = (int)s_lo, hi = (int)s_hi;
        const uint32_t m0 = bmask((int)rel, lo, hi), m1 = bmask((int)rel + 4, lo, hi), m2 = bmask((int)rel + 8, lo, hi),
                       m3 = bmask((int)rel + 12, lo, hi);
        if (m0 == 0xffffffffu) *(gwu32_t*)p = d0; else if (m0) store_partial(p, d0, m0);
        if (m1 == 0xffffffffu) *(gwu32_t*)(p + 4) = d1; else if (m1) store_partial(p + 4, d1, m1);
        if (m2 == 0xffffffffu) *(gwu32_t*)(p + 8) = d2; else if (m2) store_partial(p + 8, d2, m2);
        if (m3 == 0xffffffffu) *(gwu32_t*)(p + 12) = d3; else if (m3) store_partial(p + 12, d3, m3);
    }
}

// Lane tl's groups of the span's ng, two in flight per lane; returns the lane's accumulator.
template <bool SUB>
VPC_TM_FN uint64_t move_groups(const Span& sp, uint32_t tl, uint32_t ng) {
    uint64_t acc = 0;
    for (uint32_t g = tl; g < ng; g += 16u) {
        const bool two = g + 8u < ng;
        const Group a = load_group(sp, g);
        Group b = {0u, 0u, 0u, 0u, 0u};
        if (two) b = load_group(sp, g + 8u);
        emit_group<SUB>(sp, g, a, acc);
        if (two) emit_group<SUB>(sp, g + 8u, b, acc);
    }
    return acc;
}

// ------------------------------------------------------------------------------------------
// The piece store: register words to an address of any residue mod 4, in the widest naturally
// aligned stores the address allows -- each store's bytes cut from the words at compile-time
// positions (one instantiation per address residue: no indexed register array, no scratch).
// ------------------------------------------------------------------------------------------

// Up to 20 bytes as 5 little-endian words, held by value so that each stays a register (an array of
// them is read back in overlapping 8-B pairs that no pass splits again, and lands in LDS).
struct Piece {
    uint32_t w0, w1, w2, w3, w4;
};

template <int K>
__device__ __forceinline__ uint32_t piece_word(const Piece w) {
    return K == 0 ? w.w0 : K == 1 ? w.w1 : K == 2 ? w.w2 : K == 3 ? w.w3 : K == 4 ? w.w4 : 0u;
}

// bytes [POS, POS + 4) of a piece (bytes past it: 0)
template <int POS>
__device__ __forceinline__ uint32_t piece_bytes(const Piece w) {
    constexpr int k = POS >> 2, sh = (POS & 3) * 8;
    const uint32_t lo = piece_word<k>(w);
    if constexpr (sh == 0) return lo;
    else return (lo >> sh) | (piece_word<k + 1>(w) << (32 - sh));
}

// NB bytes of a piece to p, R = p & 3: bytes and a halfword up to the first 4-B aligned address,
// dwords, then the tail -- every store naturally aligned
template <int R, int NB, int POS = 0>
__device__ __forceinline__ void store_piece(uint8_t* p, const Piece w) {
    if constexpr (POS < NB) {
        constexpr int a = (R + POS) & 3;
        if constexpr (a == 0 && NB - POS >= 4) {
            *(gwu32_t*)(p + POS) = piece_bytes<POS>(w);
            store_piece<R, NB, POS + 4>(p, w);
        } else if constexpr ((a & 1) == 0 && NB - POS >= 2) {
            *(gwu16_t*)(p + POS) = (uint16_t)piece_bytes<POS>(w);
            store_piece<R, NB, POS + 2>(p, w);
        } else {
            *(gwu8_t*)(p + POS) = (uint8_t)piece_bytes<POS>(w);
            store_piece<R, NB, POS + 1>(p, w);
        }
    }
}

template <int NB>
__device__ __forceinline__ void store_piece_any(uint8_t* p, const Piece w) {
    switch ((uint32_t)(uintptr_t)p & 3u) {
    case 0: store_piece<0, NB>(p, w); break;
    case 1: store_piece<1, NB>(p, w); break;
    case 2: store_piece<2, NB>(p, w); break;
    default: store_piece<3, NB>(p, w); break;
    }
}

}  // namespace vpcsum
