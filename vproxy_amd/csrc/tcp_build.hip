// tcp_build.hip -- k_tcp_build (vpcsum_tcp_build_async): finished TCP data segments from "connection
// header + payload run".  Per record, the payload is read once from the send buffer, written once
// into the TX frame and added to the segment's one's complement accumulator between the two; the
// headers are generated in registers from the 64-B template and stored, with both sums, after the
// team's reduction.  No second kernel, no re-read of the written frame.
//
// Shape: a team of 8 lanes per record (K2's shape for frames), 16 B per lane and step.  The steps
// follow the DESTINATION's 16-B grid: group g covers [Pd + 16 g, +16), Pd the payload's first
// address rounded down to 16, so every interior group leaves in one aligned 16-B store.  Source and
// destination are independent modulo 16: the bytes of group g lie at s0 + 16 g in the source, s0 of
// any alignment.  They are loaded as the five 4-B aligned dwords W[4g .. 4g+4] around them (one
// 16-B load at 4-B alignment and one dword; the dword only when s0 is not 4-B aligned) and brought
// into place with v_alignbyte by s0 & 3.  Nothing assumes unaligned access.
//
// Edges: a group that is not all payload -- the first and the last of a record -- loads only those
// of its source dwords that hold a payload byte of this record (so no load can cross into a page
// the payload does not touch, and no 16-B load reaches past the last such dword), masks each
// destination dword to its payload bytes for the sum, and stores partial dwords byte by byte
// (halfwords where both bytes are payload).  No store falls outside [frame_off, frame_off + L).
//
// Sums: the accumulator is 64-bit per lane (65,515 bytes of 0xff are 2,048 dwords per lane), folded
// once (device_common.h fold64 / fold32).  Summing destination-aligned dwords makes the byte parity
// a per-record constant: the TCP header starts at an even offset of the segment, so the payload's
// sum is byte-swapped against the header words' exactly when its first address is odd.
//
// Header: lane 0 stores the Ethernet header, lanes 1..3 one 20-byte piece each of the IP and TCP
// headers, every piece from registers under compile-time indices in the widest naturally aligned
// stores its address allows (flow.hip store_macs' idiom, one instantiation per address residue).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "tcp_build.h"

namespace vpcsum {

namespace {

typedef uint32_t tb_u32x4a4_t __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const tb_u32x4a4_t tb_g128a4_t;
typedef __attribute__((address_space(1))) const uint32_t tb_g32_t;
typedef __attribute__((address_space(1))) u32x4_t tb_gw128_t;
typedef __attribute__((address_space(1))) uint32_t tb_gw32_t;
typedef __attribute__((address_space(1))) uint16_t tb_gw16_t;
typedef __attribute__((address_space(1))) uint8_t tb_gw8_t;

template <int CTRL>
__device__ __forceinline__ uint32_t tb_dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// the sum over a team of 8 consecutive lanes, in every lane of it
__device__ __forceinline__ uint32_t tb_team_sum(uint32_t v) {
    v = tb_dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
    v = tb_dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
    v = tb_dpp_add<0x141>(v);   // row_half_mirror
    return v;
}

// A header piece: up to 20 bytes as 5 little-endian words, held by value so that each stays a register
// (an array of them is read back in overlapping 8-B pairs that no pass splits again, and lands in LDS).
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
// dwords, then the tail -- every store naturally aligned, positions known at compile time
template <int R, int NB, int POS = 0>
__device__ __forceinline__ void store_piece(uint8_t* p, const Piece w) {
    if constexpr (POS < NB) {
        constexpr int a = (R + POS) & 3;
        if constexpr (a == 0 && NB - POS >= 4) {
            *(tb_gw32_t*)(p + POS) = piece_bytes<POS>(w);
            store_piece<R, NB, POS + 4>(p, w);
        } else if constexpr ((a & 1) == 0 && NB - POS >= 2) {
            *(tb_gw16_t*)(p + POS) = (uint16_t)piece_bytes<POS>(w);
            store_piece<R, NB, POS + 2>(p, w);
        } else {
            *(tb_gw8_t*)(p + POS) = (uint8_t)piece_bytes<POS>(w);
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

// the bytes of dword v that mask m names (not all four, at least one) to the 4-B aligned address a
__device__ __forceinline__ void store_partial(uint8_t* a, uint32_t v, uint32_t m) {
    if ((m & 0xffffu) == 0xffffu) {
        *(tb_gw16_t*)a = (uint16_t)v;
    } else {
        if (m & 0xffu) *(tb_gw8_t*)a = (uint8_t)v;
        if (m & 0xff00u) *(tb_gw8_t*)(a + 1) = (uint8_t)(v >> 8);
    }
    if ((m >> 16) == 0xffffu) {
        *(tb_gw16_t*)(a + 2) = (uint16_t)(v >> 16);
    } else {
        if (m & 0xff0000u) *(tb_gw8_t*)(a + 2) = (uint8_t)(v >> 16);
        if (m & 0xff000000u) *(tb_gw8_t*)(a + 3) = (uint8_t)(v >> 24);
    }
}

// What a lane needs to move the payload's groups.  Byte offsets are relative to `sa` in the source
// and to `pd` in the destination, the same number on both sides.
struct Span {
    const uint8_t* sa;   // 4-B aligned: source dword k is at sa + 4 k
    uint8_t* pd;         // 16-B aligned: group g is at pd + 16 g
    uint32_t sh;         // the source bytes of group g start at sa + 16 g + sh
    uint32_t lead;       // the payload is destination bytes [lead, lead + len)
    uint32_t len;
    uint32_t k_lo, k_hi; // the source dwords that hold a payload byte (len > 0)
};

struct Group {
    uint32_t w0, w1, w2, w3, w4;
};

__device__ __forceinline__ bool group_inner(const Span& sp, uint32_t g) {
    return g * 16u >= sp.lead && g * 16u + 16u <= sp.lead + sp.len;
}

__device__ __forceinline__ Group load_group(const Span& sp, uint32_t g) {
    Group r;
    const uint8_t* q = sp.sa + (size_t)g * 16u;
    if (group_inner(sp, g)) {
        // all 16 bytes are payload: W[4g..4g+3] each hold some of them, W[4g+4] too when sh != 0
        const tb_u32x4a4_t v = __builtin_nontemporal_load((tb_g128a4_t*)q);
        r.w0 = v.x; r.w1 = v.y; r.w2 = v.z; r.w3 = v.w;
        r.w4 = sp.sh ? __builtin_nontemporal_load((tb_g32_t*)(q + 16)) : 0u;
    } else {
        const uint32_t k = g * 4u;
        r.w0 = (k >= sp.k_lo && k <= sp.k_hi) ? __builtin_nontemporal_load((tb_g32_t*)q) : 0u;
        r.w1 = (k + 1 >= sp.k_lo && k + 1 <= sp.k_hi) ? __builtin_nontemporal_load((tb_g32_t*)(q + 4)) : 0u;
        r.w2 = (k + 2 >= sp.k_lo && k + 2 <= sp.k_hi) ? __builtin_nontemporal_load((tb_g32_t*)(q + 8)) : 0u;
        r.w3 = (k + 3 >= sp.k_lo && k + 3 <= sp.k_hi) ? __builtin_nontemporal_load((tb_g32_t*)(q + 12)) : 0u;
        r.w4 = (k + 4 >= sp.k_lo && k + 4 <= sp.k_hi) ? __builtin_nontemporal_load((tb_g32_t*)(q + 16)) : 0u;
    }
    return r;
}

// shift the group into place, add it, store it
__device__ __forceinline__ void emit_group(const Span& sp, uint32_t g, const Group& r, uint64_t& acc) {
    uint32_t d0 = __builtin_amdgcn_alignbyte(r.w1, r.w0, sp.sh);
    uint32_t d1 = __builtin_amdgcn_alignbyte(r.w2, r.w1, sp.sh);
    uint32_t d2 = __builtin_amdgcn_alignbyte(r.w3, r.w2, sp.sh);
    uint32_t d3 = __builtin_amdgcn_alignbyte(r.w4, r.w3, sp.sh);
    uint8_t* p = sp.pd + (size_t)g * 16u;
    if (group_inner(sp, g)) {
        acc += (uint64_t)d0 + d1 + d2 + d3;
        u32x4_t o;
        o.x = d0; o.y = d1; o.z = d2; o.w = d3;
        *(tb_gw128_t*)p = o;
    } else {
        const int rel = (int)(g * 16u), lo = (int)sp.lead, hi = (int)(sp.lead + sp.len);
        const uint32_t m0 = bmask(rel, lo, hi), m1 = bmask(rel + 4, lo, hi), m2 = bmask(rel + 8, lo, hi),
                       m3 = bmask(rel + 12, lo, hi);
        d0 &= m0; d1 &= m1; d2 &= m2; d3 &= m3;
        acc += (uint64_t)d0 + d1 + d2 + d3;
        if (m0 == 0xffffffffu) *(tb_gw32_t*)p = d0; else if (m0) store_partial(p, d0, m0);
        if (m1 == 0xffffffffu) *(tb_gw32_t*)(p + 4) = d1; else if (m1) store_partial(p + 4, d1, m1);
        if (m2 == 0xffffffffu) *(tb_gw32_t*)(p + 8) = d2; else if (m2) store_partial(p + 8, d2, m2);
        if (m3 == 0xffffffffu) *(tb_gw32_t*)(p + 12) = d3; else if (m3) store_partial(p + 12, d3, m3);
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_tcp_build(uint8_t* __restrict__ dst, uint64_t dst_len,
                                                  const uint8_t* __restrict__ src, uint64_t src_len,
                                                  const vpcsum_tcphdr_t* __restrict__ hdrs, uint32_t n_hdr,
                                                  const vpcsum_tcpseg_t* __restrict__ segs, uint32_t n,
                                                  uint32_t* __restrict__ frame_len_out, uint32_t* __restrict__ out,
                                                  uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = tid >> 3;            // one team of 8 lanes per record
    const uint32_t tl = threadIdx.x & 7u;
    if (i >= n) return;                     // whole teams leave: no cross-lane step misses a lane it needs

    // the record (32 B at 8-B alignment), the same two loads in every lane of the team
    const tb_u32x4a4_t ra = *(tb_g128a4_t*)(segs + i);
    const tb_u32x4a4_t rb = *(tb_g128a4_t*)((const uint8_t*)(segs + i) + 16);
    const uint64_t frame_off = ((uint64_t)ra.y << 32) | ra.x, data_off = ((uint64_t)ra.w << 32) | ra.z;
    const uint32_t seq = rb.x, hdr = rb.y, frame_cap = rb.z;
    const uint32_t data_len = rb.w & 0xffffu, flags = (rb.w >> 16) & 0xffu, rsv = rb.w >> 24;

    // a refused record loads its own words and, when it names one, its template: nothing else
    bool ok = tcp_build_seg_ok(hdr, n_hdr, flags, rsv);
    uint32_t t[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const uint8_t* hp = (const uint8_t*)(hdrs + hdr);
        const tb_u32x4a4_t h0 = *(tb_g128a4_t*)hp, h1 = *(tb_g128a4_t*)(hp + 16), h2 = *(tb_g128a4_t*)(hp + 32),
                           h3 = *(tb_g128a4_t*)(hp + 48);
        t[0] = h0.x; t[1] = h0.y; t[2] = h0.z; t[3] = h0.w;
        t[4] = h1.x; t[5] = h1.y; t[6] = h1.z; t[7] = h1.w;
        t[8] = h2.x; t[9] = h2.y; t[10] = h2.z; t[11] = h2.w;
        t[12] = h3.x; t[13] = h3.y; t[14] = h3.z; t[15] = h3.w;
        ok = tcp_build_hdr_ok(t) && tcp_build_fits(t, frame_off, data_off, frame_cap, data_len, dst_len, src_len);
    }
    if (!ok) {
        if (tl == 0) {
            frame_len_out[i] = 0u;
            if (out) out[i] = 0u;
            if (status) status[i] = (uint8_t)VPCSUM_S_BAD_DESC;
        }
        return;
    }

    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t l2 = tb_l2_len(t), H = tcp_build_header_len(t);
    uint8_t* const frame = dst + frame_off;
    uint8_t* const pay = frame + H;

    // the payload, group by group
    Span sp;
    sp.len = data_len;
    sp.lead = (uint32_t)(uintptr_t)pay & 15u;
    sp.pd = pay - sp.lead;
    const uintptr_t s0 = (uintptr_t)(src + data_off) - sp.lead;
    sp.sh = (uint32_t)s0 & 3u;
    sp.sa = (const uint8_t*)(s0 - sp.sh);
    sp.k_lo = (sp.lead + sp.sh) >> 2;
    sp.k_hi = (sp.lead + sp.sh + data_len - 1u) >> 2;   // read only when data_len > 0
    const uint32_t ng = data_len ? (sp.lead + data_len + 15u) >> 4 : 0u;
    uint64_t acc = 0;
    for (uint32_t g = tl; g < ng; g += 16u) {   // two groups in flight per lane
        const bool two = g + 8u < ng;
        const Group a = load_group(sp, g);
        Group b = {0u, 0u, 0u, 0u, 0u};
        if (two) b = load_group(sp, g + 8u);
        emit_group(sp, g, a, acc);
        if (two) emit_group(sp, g + 8u, b, acc);
    }
    // the payload's sum in the header words' byte order: its dwords lie on the destination's grid,
    // the TCP header starts on an even byte of the segment
    uint32_t ps = fold32(tb_team_sum(fold64(acc)));
    if ((uintptr_t)pay & 1u) ps = bswap16(ps);

    // the header: every lane of the team holds all of it
    TcpBuildWords w;
    tcp_build_words(t, seq, data_len, flags, w);
    const uint32_t ip_field = v4 ? 0xffffu - fold64(tcp_build_ip_header_sum(w)) : 0u;
    const uint32_t l4_field = 0xffffu - fold64(tcp_build_l4_header_sum(t, w, data_len) + ps);
    tcp_build_set_sums(w, v4, ip_field, l4_field);

    if (tl == 0) {
        if (l2) {
            store_piece_any<14>(frame, Piece{w.eth[0], w.eth[1], w.eth[2], w.eth[3], 0u});
        }
        frame_len_out[i] = H + data_len;
        if (out) out[i] = bswap16(ip_field) | (bswap16(l4_field) << 16);
        if (status) status[i] = (uint8_t)VPCSUM_S_DONE;
    } else if (tl == 1) {
        // 20-byte pieces of IP ‖ TCP, a lane each -- IPv4: ip, tcp; IPv6: ip[0..4], ip[5..9], tcp.  (One
        // branch per piece, every word under a compile-time index.)
        store_piece_any<20>(frame + l2, Piece{w.ip[0], w.ip[1], w.ip[2], w.ip[3], w.ip[4]});
    } else if (tl == 2 && !v4) {
        store_piece_any<20>(frame + l2 + 20u, Piece{w.ip[5], w.ip[6], w.ip[7], w.ip[8], w.ip[9]});
    } else if (tl == (v4 ? 2u : 3u)) {
        store_piece_any<20>(frame + l2 + (v4 ? 20u : 40u), Piece{w.tcp[0], w.tcp[1], w.tcp[2], w.tcp[3], w.tcp[4]});
    }
}

hipError_t launch_tcp_build(uint8_t* dst, uint64_t dst_len, const uint8_t* src, uint64_t src_len,
                            const vpcsum_tcphdr_t* hdrs, uint32_t n_hdr, const vpcsum_tcpseg_t* segs, uint32_t n,
                            uint32_t* frame_len_out, uint32_t* out, uint8_t* status, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_tcp_build, dim3(g), dim3(256), 0, stream, dst, dst_len, src, src_len, hdrs, n_hdr, segs, n,
                       frame_len_out, out, status);
    return hipGetLastError();
}

}  // namespace vpcsum
