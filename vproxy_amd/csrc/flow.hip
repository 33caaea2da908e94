// flow.hip -- the NAT flow table's lookup kernels (vpcsum_flow_lookup_async, _fp_async): per packet,
// the tuple the parse wrote is hashed, its home slot and up to max_probe more are read, and the flow's
// vpcsum_nat_t entry -- or zeros -- is written for the rewrite kernel that runs next on the stream
// (k_flowfp: the flow's Fastpath too); and the L2 write that follows the rewrite (k_l2_forward).
//
// Shape: a team of 8 lanes per packet, the shape K2 uses for frames.  A slot is one 128-B line
// (flow_table.h FlowSlot) and each lane of the team loads 16 B of it, so one load instruction
// brings a whole line per packet and probe, 8 packets per wave:
//   lane 0  key.src                      compared with the tuple's src
//   lane 1  key.dst                      ... dst
//   lane 2  ports, version, protocol | flow id | occupied
//   lanes 3..5  the 48-B entry: on a HIT stored as it was loaded, 3 x 16 B contiguous
//   lane 6  cookie, padding: loaded (the line comes whole) and not used
//   lane 7  the flow's Fastpath (vpcsum_fastpath_t): stored by k_flowfp, not used by k_flow_lookup
// The tuple is loaded in the same layout (lanes 0..2), so the key compare is lane-local and the
// team's verdict one ballot; the hash is the sum of per-word mixes (flow_table.h), each lane mixing
// the words it holds, added across the team with three shuffles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "flow_table.h"
#include "internal.h"
#include "team_move.h"

namespace vpcsum {

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The lookup of one packet by its team, whole: the body of both kernels, so that the two cannot
// drift.  FP (a constant at each call): lane 7 also stores the flow's Fastpath.
template <bool FP>
__device__ __forceinline__ void flow_lookup_team(const FlowSlot* __restrict__ slots, uint32_t mask, uint32_t max_probe,
                                                 uint8_t* __restrict__ touched, const vpcsum_tuple_t* __restrict__ tuples,
                                                 uint32_t n, vpcsum_nat_t* __restrict__ rw_out,
                                                 uint8_t* __restrict__ verdict_out, vpcsum_fastpath_t* __restrict__ fp_out) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t pkt = tid >> 3;          // one team of 8 lanes per packet
    const uint32_t l8 = threadIdx.x & 7u;   // the lane's 16-B piece of a slot
    const uint32_t team_shift = threadIdx.x & 56u;   // the team's first lane in its wave
    const bool valid = pkt < n;             // whole teams: n teams, 8 lanes each

    // the tuple, in the slot's layout: lanes 0 and 1 take 16 B, lane 2 the last 8 (read once: non-temporal)
    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    const uint8_t* tp = (const uint8_t*)(tuples + (valid ? pkt : 0u)) + l8 * 16u;
    if (valid && l8 < 2) {
        const u32x4a4_t v = __builtin_nontemporal_load((gu32x4a4_t*)tp);
        t0 = v.x; t1 = v.y; t2 = v.z; t3 = v.w;
    } else if (valid && l8 == 2) {
        const u32x2a4_t v = __builtin_nontemporal_load((gu32x2a4_t*)tp);
        t0 = v.x;
        t1 = v.y;
    }
    // lane 2's second word: l3_ver | l4_proto << 8 | tcp_flags << 16 | rsv << 24; the key stops before the flags
    const uint32_t meta = (uint32_t)__shfl((int)t1, (int)(team_shift + 2u), 64);
    if (l8 == 2) t1 &= 0xffffu;
    const uint32_t ver = meta & 0xffu, proto = (meta >> 8) & 0xffu, flags = (meta >> 16) & 0xffu;

    // hash: each lane mixes its two 64-bit words (lane 2: one; lanes 3..7: none), the team adds them
    uint64_t h = 0;
    if (l8 < 3) {
        h = flow_word_hash(((uint64_t)t1 << 32) | t0, (int)(2u * l8));
        if (l8 < 2) h += flow_word_hash(((uint64_t)t3 << 32) | t2, (int)(2u * l8 + 1u));
    }
    h += shfl_xor_u64(h, 1);
    h += shfl_xor_u64(h, 2);
    h += shfl_xor_u64(h, 4);
    uint32_t idx = (uint32_t)flow_mix(h) & mask;

    // a refused frame (l3_ver 0) and anything but TCP / UDP is in no table: no probe
    bool probing = valid && ver != 0u && (proto == 6u || proto == 17u);
    bool found = false;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    // team-uniform control flow: the 8 lanes of a team leave the loop together, so a ballot's 8 bits
    // of the team are those of live lanes
    for (uint32_t p = 0; probing && p <= max_probe; ++p) {
        const u32x4_t v = *(gu32x4_t*)((const uint8_t*)(slots + idx) + l8 * 16u);
        s0 = v.x; s1 = v.y; s2 = v.z; s3 = v.w;
        // lanes 0, 1: 16 key bytes; lane 2: 6 key bytes (the slot's flags / rsv are 0) and occupied; 3..7: nothing to compare
        const bool same = l8 < 2 ? (s0 == t0 && s1 == t1 && s2 == t2 && s3 == t3)
                        : l8 == 2 ? (s0 == t0 && s1 == t1 && s3 != 0u) : true;
        const bool empty = l8 == 2 && s3 == 0u;
        const uint32_t m_same = (uint32_t)(__ballot(same) >> team_shift) & 0xffu;
        const uint32_t m_empty = (uint32_t)(__ballot(empty) >> team_shift) & 0xffu;
        found = m_same == 0xffu;
        if (found || m_empty != 0u) probing = false;
        idx = (idx + 1u) & mask;
    }

    if (!valid) return;
    const bool punt = found && proto == 6u && (flags & 0x07u) != 0u;   // FIN | SYN | RST: the host's packet
    const bool hit = found && !punt;
    if (l8 >= 3 && l8 < 6) {
        // the entry as loaded, or zeros (mask 0: the rewrite kernel answers S_DONE and writes nothing)
        u32x4a4_t o;
        o.x = hit ? s0 : 0u; o.y = hit ? s1 : 0u; o.z = hit ? s2 : 0u; o.w = hit ? s3 : 0u;
        *(gwu32x4a4_t*)((uint8_t*)(rw_out + pkt) + (l8 - 3u) * 16u) = o;
    } else if (l8 == 2) {
        if (hit) touched[s2] = 1;   // s2: the flow id; a plain byte store of a constant, idempotent
    } else if (l8 == 0) {
        verdict_out[pkt] = hit ? (uint8_t)VPCSUM_FLOW_HIT : punt ? (uint8_t)VPCSUM_FLOW_PUNT : (uint8_t)VPCSUM_FLOW_MISS;
    } else if (FP && l8 == 7) {
        // the flow's Fastpath (slot bytes 112..127) as loaded, or zeros
        u32x4a4_t o;
        o.x = hit ? s0 : 0u; o.y = hit ? s1 : 0u; o.z = hit ? s2 : 0u; o.w = hit ? s3 : 0u;
        *(gwu32x4a4_t*)(fp_out + pkt) = o;
    }
}

__global__ __launch_bounds__(256) void k_flow_lookup(const FlowSlot* __restrict__ slots, uint32_t mask, uint32_t max_probe,
                                                    uint8_t* __restrict__ touched,
                                                    const vpcsum_tuple_t* __restrict__ tuples, uint32_t n,
                                                    vpcsum_nat_t* __restrict__ rw_out, uint8_t* __restrict__ verdict_out) {
    flow_lookup_team<false>(slots, mask, max_probe, touched, tuples, n, rw_out, verdict_out, nullptr);
}

// The lookup that also hands out the flow's Fastpath: lane 7 holds the slot's bytes 112..127, the
// vpcsum_fastpath_t, and stores them as loaded on a HIT, zeros otherwise.
__global__ __launch_bounds__(256) void k_flowfp(const FlowSlot* __restrict__ slots, uint32_t mask, uint32_t max_probe,
                                               uint8_t* __restrict__ touched, const vpcsum_tuple_t* __restrict__ tuples,
                                               uint32_t n, vpcsum_nat_t* __restrict__ rw_out,
                                               uint8_t* __restrict__ verdict_out, vpcsum_fastpath_t* __restrict__ fp_out) {
    flow_lookup_team<true>(slots, mask, max_probe, touched, tuples, n, rw_out, verdict_out, fp_out);
}

// ------------------------------------------------------------------------------------------
// The L2 write (vpcsum_l2_forward_async): one lane per frame.  A frame's 12 address bytes start at
// arena + frame_off, of any alignment; they are held as three little-endian dwords and leave in the
// widest naturally aligned stores the address allows -- 3 stores at a 4-B aligned address, 4 at an
// even one, 5 at an odd one (team_move.h store_piece_any).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_l2_forward(uint8_t* __restrict__ arena, uint64_t arena_len,
                                                   const uint64_t* __restrict__ frame_off,
                                                   const uint32_t* __restrict__ frame_len,
                                                   const uint8_t* __restrict__ verdict, const uint8_t* __restrict__ status,
                                                   const vpcsum_fastpath_t* __restrict__ fp, uint32_t n,
                                                   uint32_t* __restrict__ port_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t off = frame_off[i];
    const uint32_t len = frame_len[i];
    const uint32_t vd = verdict[i], st = status[i];
    const u32x4a4_t f = *(gu32x4a4_t*)(fp + i);   // dst[6] src[6] | port
    // the frame holds an Ethernet header inside the arena (the sum cannot wrap: off <= arena_len first)
    const bool inside = len >= 14u && off <= arena_len && (uint64_t)len <= arena_len - off;
    const bool go = inside && vd == VPCSUM_FLOW_HIT && (st & (VPCSUM_S_DONE | VPCSUM_S_BAD_DESC)) == VPCSUM_S_DONE && f.w != 0u;
    port_out[i] = go ? f.w : 0u;
    if (!go) return;
    store_piece_any<12>(arena + off, Piece{f.x, f.y, f.z, 0u, 0u});
}

hipError_t launch_flow_lookup(const void* slots, uint32_t mask, uint32_t max_probe, uint8_t* touched,
                              const vpcsum_tuple_t* tuples, uint32_t n, vpcsum_nat_t* rw_out, uint8_t* verdict_out,
                              vpcsum_fastpath_t* fp_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + 31u) / 32u;   // 256 threads: 32 teams
    if (fp_out)
        hipLaunchKernelGGL(k_flowfp, dim3(g), dim3(256), 0, stream, (const FlowSlot*)slots, mask, max_probe, touched, tuples, n,
                           rw_out, verdict_out, fp_out);
    else
        hipLaunchKernelGGL(k_flow_lookup, dim3(g), dim3(256), 0, stream, (const FlowSlot*)slots, mask, max_probe, touched,
                           tuples, n, rw_out, verdict_out);
    return hipGetLastError();
}

hipError_t launch_l2_forward(uint8_t* arena, uint64_t arena_len, const uint64_t* frame_off, const uint32_t* frame_len,
                             const uint8_t* verdict, const uint8_t* status, const vpcsum_fastpath_t* fp, uint32_t n,
                             uint32_t* port_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_l2_forward, dim3((n + 255u) / 256u), dim3(256), 0, stream, arena, arena_len, frame_off, frame_len,
                       verdict, status, fp, n, port_out);
    return hipGetLastError();
}

}  // namespace vpcsum
