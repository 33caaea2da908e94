// tcp_recv.hip -- k_tcp_recv (vpcsum_tcp_recv_async) and k_tcp_digest (vpcsum_tcp_digest_async): the
// receive side of the userspace TCP stack, tcp_build.hip run the other way.  Per record the segment is
// read once; every byte is added to the TCP sum and, when it is payload past the record's `skip`,
// stored into the receive buffer from the register that summed it.  No second pass over the payload.
//
// Shape: a team of 8 lanes per record, 16 B per lane and step, as k_tcp_build.  The steps follow ONE
// 16-B grid for the sum and the store: the destination's.  The whole segment is laid on it through a
// virtual destination address V0 = dst + dst_off - (hlen + skip) of segment byte 0 -- an integer,
// never dereferenced below dst + dst_off -- so that payload byte `skip` falls on dst + dst_off and
// every interior group of the stored range leaves in one aligned 16-B store.  Group g covers the
// grid's bytes [16 g, 16 g + 16), the segment [lead, lead + seg_len) of them (lead = V0 & 15), the
// stored range [s_lo, s_hi) = [lead + hlen + skip, lead + seg_len).  The TCP header and the skipped
// prefix are groups that are summed and masked out of the store: emit_group has a sum bound and a
// second, store-only bound.  A record that stores nothing (verify only, or skip == data_len) takes the
// source's own grid (V0 = the segment's address): its loads are aligned and it has no store bound.
//
// Source loads: the bytes of group g lie at s0 + 16 g, s0 of any alignment relative to the grid.  They
// are loaded as the five 4-B aligned dwords around them and shifted with v_alignbyte by s0 & 3.  A
// dword is loaded only when it holds a byte of the segment [l3_off + l4_off, l3_off + l3_len): no
// load crosses into a page the segment does not touch, and L2 padding after l3_len is neither read
// nor summed (edge groups load dword by dword under k_lo / k_hi and mask to the segment).  Besides
// that stream every lane reads three header bytes of its record on their own: byte 12 (the data
// offset, all a refused record may read) and bytes 16..17 (the stored field).
//
// Sums: 64-bit per lane (65,515 bytes of 0xff are 2,048 dwords per lane), folded once
// (device_common.h fold64 / fold32).  Summing grid-aligned dwords makes the byte parity one constant
// per record: the folded sum is byte-swapped when V0 is odd.  The stored checksum field is part of
// that sum and is taken out by one's complement subtraction (+ 0xffff - field), so `out` holds the
// recomputed value and the compare is exact; the sum cannot be 0 (it holds protocol 6), so the result
// is the representative 1..0xffff that summing with a zeroed field gives.  The pseudo-header
// addresses are summed from the L3 header where it lies, a shifted dword per lane; with F_IP lane 7
// sums the l4_off header bytes with the field masked (an all-zero header must give 0xffff).
//
// Early exit: i >= n, refused records and every other branch on a record's words are uniform over
// the team, so whole teams leave together and no DPP step misses a lane it needs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "tcp_recv.h"

namespace vpcsum {

namespace {

typedef uint32_t tr_u32x4a4_t __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const tr_u32x4a4_t tr_g128a4_t;
typedef __attribute__((address_space(1))) const uint32_t tr_g32_t;
typedef __attribute__((address_space(1))) const uint8_t tr_g8_t;
typedef __attribute__((address_space(1))) u32x4_t tr_gw128_t;
typedef __attribute__((address_space(1))) uint32_t tr_gw32_t;
typedef __attribute__((address_space(1))) uint16_t tr_gw16_t;
typedef __attribute__((address_space(1))) uint8_t tr_gw8_t;

template <int CTRL>
__device__ __forceinline__ uint32_t tr_dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// the sum over a team of 8 consecutive lanes, in every lane of it
__device__ __forceinline__ uint32_t tr_team_sum(uint32_t v) {
    v = tr_dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
    v = tr_dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
    v = tr_dpp_add<0x141>(v);   // row_half_mirror
    return v;
}

// the bytes of dword v that mask m names (not all four, at least one) to the 4-B aligned address a
__device__ __forceinline__ void store_partial(uintptr_t a, uint32_t v, uint32_t m) {
    if ((m & 0xffffu) == 0xffffu) {
        *(tr_gw16_t*)a = (uint16_t)v;
    } else {
        if (m & 0xffu) *(tr_gw8_t*)a = (uint8_t)v;
        if (m & 0xff00u) *(tr_gw8_t*)(a + 1) = (uint8_t)(v >> 8);
    }
    if ((m >> 16) == 0xffffu) {
        *(tr_gw16_t*)(a + 2) = (uint16_t)(v >> 16);
    } else {
        if (m & 0xff0000u) *(tr_gw8_t*)(a + 2) = (uint8_t)(v >> 16);
        if (m & 0xff000000u) *(tr_gw8_t*)(a + 3) = (uint8_t)(v >> 24);
    }
}

// What a lane needs to move the segment's groups.  Byte offsets are relative to `sa` in the source
// and to the grid base `pd` on the destination side, the same number on both.
struct Span {
    uintptr_t sa;        // 4-B aligned: source dword k is at sa + 4 k
    uintptr_t pd;        // 16-B aligned, virtual: group g is at pd + 16 g (only [s_lo, s_hi) of it exists)
    uint32_t sh;         // the source bytes of group g start at sa + 16 g + sh
    uint32_t lo, hi;     // the segment is grid bytes [lo, hi): what is summed
    uint32_t s_lo, s_hi; // the stored range, inside [lo, hi); s_lo == s_hi: nothing is stored
    uint32_t k_lo, k_hi; // the source dwords that hold a segment byte
};

struct Group {
    uint32_t w0, w1, w2, w3, w4;
};

__device__ __forceinline__ bool group_inner(const Span& sp, uint32_t g) {
    return g * 16u >= sp.lo && g * 16u + 16u <= sp.hi;
}

__device__ __forceinline__ Group load_group(const Span& sp, uint32_t g) {
    Group r;
    const uintptr_t q = sp.sa + (size_t)g * 16u;
    if (group_inner(sp, g)) {
        // all 16 bytes are segment: W[4g..4g+3] each hold some of them, W[4g+4] too when sh != 0
        const tr_u32x4a4_t v = __builtin_nontemporal_load((tr_g128a4_t*)q);
        r.w0 = v.x; r.w1 = v.y; r.w2 = v.z; r.w3 = v.w;
        r.w4 = sp.sh ? __builtin_nontemporal_load((tr_g32_t*)(q + 16)) : 0u;
    } else {
        const uint32_t k = g * 4u;
        r.w0 = (k >= sp.k_lo && k <= sp.k_hi) ? __builtin_nontemporal_load((tr_g32_t*)q) : 0u;
        r.w1 = (k + 1 >= sp.k_lo && k + 1 <= sp.k_hi) ? __builtin_nontemporal_load((tr_g32_t*)(q + 4)) : 0u;
        r.w2 = (k + 2 >= sp.k_lo && k + 2 <= sp.k_hi) ? __builtin_nontemporal_load((tr_g32_t*)(q + 8)) : 0u;
        r.w3 = (k + 3 >= sp.k_lo && k + 3 <= sp.k_hi) ? __builtin_nontemporal_load((tr_g32_t*)(q + 12)) : 0u;
        r.w4 = (k + 4 >= sp.k_lo && k + 4 <= sp.k_hi) ? __builtin_nontemporal_load((tr_g32_t*)(q + 16)) : 0u;
    }
    return r;
}

// shift the group into place, add what is segment, store what is in the stored range
__device__ __forceinline__ void emit_group(const Span& sp, uint32_t g, const Group& r, uint64_t& acc) {
    uint32_t d0 = __builtin_amdgcn_alignbyte(r.w1, r.w0, sp.sh);
    uint32_t d1 = __builtin_amdgcn_alignbyte(r.w2, r.w1, sp.sh);
    uint32_t d2 = __builtin_amdgcn_alignbyte(r.w3, r.w2, sp.sh);
    uint32_t d3 = __builtin_amdgcn_alignbyte(r.w4, r.w3, sp.sh);
    const uint32_t rel = g * 16u;
    if (!group_inner(sp, g)) {
        const int lo = (int)sp.lo, hi = (int)sp.hi;
        d0 &= bmask((int)rel, lo, hi);
        d1 &= bmask((int)rel + 4, lo, hi);
        d2 &= bmask((int)rel + 8, lo, hi);
        d3 &= bmask((int)rel + 12, lo, hi);
    }
    acc += (uint64_t)d0 + d1 + d2 + d3;
    const uintptr_t p = sp.pd + (size_t)rel;
    if (rel >= sp.s_lo && rel + 16u <= sp.s_hi) {
        u32x4_t o;
        o.x = d0; o.y = d1; o.z = d2; o.w = d3;
        *(tr_gw128_t*)p = o;
    } else if (rel + 16u > sp.s_lo && rel < sp.s_hi) {
        // the stored range begins or ends in this group: the store-only bound
        const int lo = (int)sp.s_lo, hi = (int)sp.s_hi;
        const uint32_t m0 = bmask((int)rel, lo, hi), m1 = bmask((int)rel + 4, lo, hi), m2 = bmask((int)rel + 8, lo, hi),
                       m3 = bmask((int)rel + 12, lo, hi);
        if (m0 == 0xffffffffu) *(tr_gw32_t*)p = d0; else if (m0) store_partial(p, d0, m0);
        if (m1 == 0xffffffffu) *(tr_gw32_t*)(p + 4) = d1; else if (m1) store_partial(p + 4, d1, m1);
        if (m2 == 0xffffffffu) *(tr_gw32_t*)(p + 8) = d2; else if (m2) store_partial(p + 8, d2, m2);
        if (m3 == 0xffffffffu) *(tr_gw32_t*)(p + 12) = d3; else if (m3) store_partial(p + 12, d3, m3);
    }
}

// bytes [p, p + 4) as a little-endian dword, p of any alignment, from the one or two 4-B aligned
// dwords that hold them
__device__ __forceinline__ uint32_t load_shifted(uintptr_t p) {
    const uint32_t sh = (uint32_t)p & 3u;
    const uintptr_t a = p - sh;
    const uint32_t lo = *(tr_g32_t*)a;
    const uint32_t hi = sh ? *(tr_g32_t*)(a + 4) : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

struct Desc {
    uint64_t l3_off;
    uint32_t l3_len, l4_off, l3_ver, l4_proto, flags;
};
__device__ __forceinline__ Desc load_desc(const vpcsum_desc_t* d) {
    const tr_u32x4a4_t v = *(tr_g128a4_t*)d;   // 16 B at 8-B alignment
    Desc r;
    r.l3_off = ((uint64_t)v.y << 32) | v.x;
    r.l3_len = v.z & 0xffffu;
    r.l4_off = v.z >> 16;
    r.l3_ver = v.w & 0xffu;
    r.l4_proto = (v.w >> 8) & 0xffu;
    r.flags = (v.w >> 16) & 0xffu;
    return r;
}

}  // namespace

__global__ __launch_bounds__(256) void k_tcp_recv(const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                 const vpcsum_desc_t* __restrict__ desc,
                                                 const vpcsum_tcprx_t* __restrict__ rx, uint32_t n,
                                                 uint8_t* __restrict__ dst, uint64_t dst_len,
                                                 uint32_t* __restrict__ stored_out, uint32_t* __restrict__ out,
                                                 uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = tid >> 3;            // one team of 8 lanes per record
    const uint32_t tl = threadIdx.x & 7u;
    if (i >= n) return;                     // whole teams leave: no cross-lane step misses a lane it needs

    // the descriptor and the record, the same two loads in every lane of the team
    const Desc d = load_desc(desc + i);
    const tr_u32x4a4_t ra = *(tr_g128a4_t*)(rx + i);
    const uint64_t dst_off = ((uint64_t)ra.y << 32) | ra.x;
    const uint32_t dst_cap = ra.z, skip = ra.w & 0xffffu, ops = (ra.w >> 16) & 0xffu, rsv = ra.w >> 24;

    // a refused record reads its own words and, when the descriptor's bounds allow, the header's byte 12
    bool ok = tcp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len) &&
              tcp_recv_ops_ok(ops, rsv);
    const uint32_t seg_len = d.l3_len - d.l4_off;
    const uintptr_t l3 = (uintptr_t)arena + d.l3_off, seg = l3 + d.l4_off;
    uint32_t hlen = 0, data_len = 0, stored = 0;
    if (ok) {
        const uint32_t b12 = *(tr_g8_t*)(seg + 12);
        ok = tcp_recv_hdr_ok(seg_len, b12, &hlen, &data_len) &&
             tcp_recv_store_ok(data_len, skip, ops, dst_off, dst_cap, dst_len, &stored);
    }
    if (!ok) {
        if (tl == 0) {
            stored_out[i] = 0u;
            if (out) out[i] = 0u;
            if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
        }
        return;
    }
    // the stored field, as it lies (little-endian domain of the segment's 16-bit words)
    const uint32_t field = (uint32_t) * (tr_g8_t*)(seg + 16) | ((uint32_t) * (tr_g8_t*)(seg + 17) << 8);

    // the grid: the destination's when bytes are stored, else the source's own
    const uintptr_t v0 = stored ? (uintptr_t)dst + dst_off - (hlen + skip) : seg;
    Span sp;
    sp.lo = (uint32_t)v0 & 15u;
    sp.hi = sp.lo + seg_len;
    sp.pd = v0 - sp.lo;
    sp.s_hi = sp.hi;
    sp.s_lo = stored ? sp.lo + hlen + skip : sp.hi;
    const uintptr_t s0 = seg - sp.lo;
    sp.sh = (uint32_t)s0 & 3u;
    sp.sa = s0 - sp.sh;
    sp.k_lo = (sp.lo + sp.sh) >> 2;
    sp.k_hi = (sp.lo + sp.sh + seg_len - 1u) >> 2;
    const uint32_t ng = (sp.hi + 15u) >> 4;   // seg_len >= 20: at least two groups' worth of bytes
    uint64_t acc = 0;
    for (uint32_t g = tl; g < ng; g += 16u) {   // two groups in flight per lane
        const bool two = g + 8u < ng;
        const Group a = load_group(sp, g);
        Group b = {0u, 0u, 0u, 0u, 0u};
        if (two) b = load_group(sp, g + 8u);
        emit_group(sp, g, a, acc);
        if (two) emit_group(sp, g + 8u, b, acc);
    }

    // the pseudo-header's addresses from the L3 header where it lies: 2 (IPv4, bytes 12..19) or 8
    // (IPv6, bytes 8..39) dwords, a lane each; they start on an even byte of the header, so their sum
    // is in the segment's own 16-bit word order
    const bool v4 = d.l3_ver == 4u;
    uint32_t ph = 0;
    if (tl < (v4 ? 2u : 8u)) {
        const uint32_t w = load_shifted(l3 + (v4 ? 12u : 8u) + 4u * tl);
        ph = (w & 0xffffu) + (w >> 16);
    }
    // the IPv4 header sum: lane 7 (it holds no address dword of an IPv4 packet), field masked
    uint32_t ipw = 0;
    if (tl == 7u && (d.flags & VPCSUM_F_IP)) {
        const uint32_t sh = (uint32_t)l3 & 3u, nw = d.l4_off >> 2;
        const uintptr_t a = l3 - sh;
        uint64_t ipacc = 0;
        uint32_t cur = *(tr_g32_t*)a, ip_field = 0;
        for (uint32_t j = 0; j < nw; ++j) {
            // the next dword: always inside the packet (the segment follows the header)
            const uint32_t nxt = (sh || j + 1u < nw) ? *(tr_g32_t*)(a + 4u * j + 4u) : 0u;
            uint32_t w = __builtin_amdgcn_alignbyte(nxt, cur, sh);
            cur = nxt;
            if (j == 2u) {
                ip_field = w >> 16;
                w &= 0xffffu;
            }
            ipacc += w;
        }
        const uint32_t ipc = 0xffffu - bswap16(fold64(ipacc));
        ipw = ipc | (bswap16(ip_field) == ipc ? 0x10000u : 0u);
    }

    uint32_t ps = fold32(tr_team_sum(fold64(acc)));
    if (v0 & 1u) ps = bswap16(ps);   // the one byte parity of the record
    ph = tr_team_sum(ph);
    ipw = tr_team_sum(ipw);          // lane 7's word in every lane
    if (tl == 0) {
        // protocol 6 and the segment length as the pseudo-header holds them; the stored field out
        const uint64_t total = (uint64_t)ps + ph + (6u << 8) + bswap16(seg_len) + (0xffffu - field);
        const uint32_t l4c = 0xffffu - bswap16(fold64(total));
        uint32_t st = VPCSUM_S_DONE;
        if (bswap16(field) == l4c) st |= VPCSUM_S_L4_OK;
        if (ipw & 0x10000u) st |= VPCSUM_S_IP_OK;
        stored_out[i] = stored;
        if (out) out[i] = (ipw & 0xffffu) | (l4c << 16);
        if (status) status[i] = (uint8_t)st;
    }
}

// A lane per descriptor: the TCP header's first 16 bytes as the 4 or 5 aligned dwords around them.
__global__ __launch_bounds__(256) void k_tcp_digest(const uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const vpcsum_desc_t* __restrict__ desc, uint32_t n,
                                                   vpcsum_tcpinfo_t* __restrict__ info) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Desc d = load_desc(desc + i);
    u32x4_t o;
    o.x = o.y = o.z = o.w = 0u;
    if (tcp_recv_desc_ok(d.l3_off, d.l3_len, d.l4_off, d.l3_ver, d.l4_proto, d.flags, arena_len)) {
        const uintptr_t seg = (uintptr_t)arena + d.l3_off + d.l4_off;
        const uint32_t sh = (uint32_t)seg & 3u;
        const uintptr_t a = seg - sh;
        const tr_u32x4a4_t v = *(tr_g128a4_t*)a;
        const uint32_t w4 = sh ? *(tr_g32_t*)(a + 16) : 0u;   // holds bytes 16 - sh .. 19 - sh: the segment has 20
        const uint32_t d1 = __builtin_amdgcn_alignbyte(v.z, v.y, sh), d2 = __builtin_amdgcn_alignbyte(v.w, v.z, sh),
                       d3 = __builtin_amdgcn_alignbyte(w4, v.w, sh);
        uint32_t hlen = 0, data_len = 0;
        if (tcp_recv_hdr_ok(d.l3_len - d.l4_off, d3 & 0xffu, &hlen, &data_len)) {
            o.x = __builtin_bswap32(d1);
            o.y = __builtin_bswap32(d2);
            o.z = bswap16(d3 >> 16) | (data_len << 16);
            o.w = hlen | (((d3 >> 8) & 0x3fu) << 8);
        }
    }
    *(tr_gw128_t*)(info + i) = o;
}

hipError_t launch_tcp_recv(const uint8_t* arena, uint64_t arena_len, const vpcsum_desc_t* desc, const vpcsum_tcprx_t* rx,
                           uint32_t n, uint8_t* dst, uint64_t dst_len, uint32_t* stored, uint32_t* out, uint8_t* status,
                           hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_tcp_recv, dim3(g), dim3(256), 0, stream, arena, arena_len, desc, rx, n, dst, dst_len, stored, out,
                       status);
    return hipGetLastError();
}

hipError_t launch_tcp_digest(const uint8_t* arena, uint64_t arena_len, const vpcsum_desc_t* desc, uint32_t n,
                             vpcsum_tcpinfo_t* info, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tcp_digest, dim3((n + 255u) / 256u), dim3(256), 0, stream, arena, arena_len, desc, n, info);
    return hipGetLastError();
}

}  // namespace vpcsum
