// tcp_burst.hip -- k_tcp_build_bursts (vpcsum_tcp_build_bursts_async): the TCP segment build with the
// stack's slicing on the device.  One record per SendingQueue.fetch() names a run of payload, its
// first sequence number and the MSS; a team of 8 lanes per FRAME of the table finds the frame's
// burst, derives the per-segment record in registers (tcp_burst.h) and runs tcp_frame.h's body, the
// one k_tcp_build runs.
//
// The search (tcp_burst.h): 9-ary over bursts[].first.  Each lane of the team probes one of a step's
// 8 pivots with a 4-byte load, the wave's ballot gives every lane its team's 8 answers, and all 8
// lanes narrow the interval alike -- so a team walks one path, leaves its loop as a whole, and
// team_sum<8> in the body sees all its lanes.  4 steps for 4,096 bursts, 6 for 131,072; consecutive
// teams of a wave mostly share a burst and probe the same lines.  The search's registers are dead
// before the body starts.  The record it lands on is checked against the frame (tcp_burst_covers)
// and against every bound before anything is built from it: an unsorted table yields refused or
// oddly attributed frames, never an access outside the frame and the burst's own source range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "tcp_burst.h"
#include "tcp_frame.h"

namespace vpcsum {

__global__ __launch_bounds__(256) void k_tcp_build_bursts(uint8_t* __restrict__ dst, uint64_t dst_len,
                                                         const uint8_t* __restrict__ src, uint64_t src_len,
                                                         const vpcsum_tcphdr_t* __restrict__ hdrs, uint32_t n_hdr,
                                                         const vpcsum_tcpburst_t* __restrict__ bursts, uint32_t n_bursts,
                                                         const uint64_t* __restrict__ frame_offs, uint32_t n_frames,
                                                         uint32_t frame_cap, uint32_t* __restrict__ frame_len_out,
                                                         uint32_t* __restrict__ out, uint8_t* __restrict__ status) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t j = tid >> 3;            // one team of 8 lanes per frame
    const uint32_t tl = threadIdx.x & 7u;
    if (j >= n_frames) return;              // whole teams leave: no cross-lane step misses a lane it needs

    // how many bursts start at or before frame j: every probe's index is below n_bursts
    const uint32_t team_shift = threadIdx.x & 56u;   // the team's first lane within its wave
    uint32_t lo = 0, hi = n_bursts;
#ifdef VPCSUM_BURST_BINARY_SEARCH
    // A/B tooling (tools/segbench.py --lib): the plain binary search, every lane of the team the same load
    (void)team_shift;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (*(gu32_t*)((const uint8_t*)(bursts + mid) + offsetof(vpcsum_tcpburst_t, first)) <= j) lo = mid + 1u;
        else hi = mid;
    }
#else
    while (lo < hi) {
        const uint8_t* pp = (const uint8_t*)(bursts + tcp_burst_pivot(lo, hi, tl)) + offsetof(vpcsum_tcpburst_t, first);
        const bool at_or_before = *(gu32_t*)pp <= j;
        const uint32_t bits = (uint32_t)(__builtin_amdgcn_ballot_w64(at_or_before) >> team_shift) & 0xffu;
        tcp_burst_narrow(lo, hi, bits);
    }
#endif
    if (lo == 0) {                          // no burst at or before it (n_bursts 0 too)
        tcp_build_refuse(j, tl, frame_len_out, out, status);
        return;
    }

    // the burst record (32 B at 8-B alignment), the same two loads in every lane of the team
    const vpcsum_tcpburst_t* bp = bursts + (lo - 1u);
    const u32x4a4_t ra = *(gu32x4a4_t*)bp;
    const u32x4a4_t rb = *(gu32x4a4_t*)((const uint8_t*)bp + 16);
    const TcpBurst b = tcp_burst_unpack(ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w);
    if (!tcp_burst_covers(b, j)) {
        tcp_build_refuse(j, tl, frame_len_out, out, status);
        return;
    }
    const u32x2a4_t fo = *(gu32x2a4_t*)(frame_offs + j);
    const uint64_t frame_off = ((uint64_t)fo.y << 32) | fo.x;
    const TcpBurstPiece p = tcp_burst_piece(b, j - b.first);

    tcp_build_frame(dst, dst_len, src, src_len, hdrs, n_hdr, j, tl, frame_off, p.data_off, p.seq, b.hdr, frame_cap, p.data_len,
                    b.flags, b.rsv, frame_len_out, out, status,
                    [&](const uint32_t (&t)[16]) { return tcp_burst_ok(t, b, frame_cap, src_len); });
}

hipError_t launch_tcp_build_bursts(uint8_t* dst, uint64_t dst_len, const uint8_t* src, uint64_t src_len,
                                   const vpcsum_tcphdr_t* hdrs, uint32_t n_hdr, const vpcsum_tcpburst_t* bursts,
                                   uint32_t n_bursts, const uint64_t* frame_off, uint32_t n_frames, uint32_t frame_cap,
                                   uint32_t* frame_len_out, uint32_t* out, uint8_t* status, hipStream_t stream) {
    if (n_frames == 0) return hipSuccess;
    const uint32_t g = (n_frames + 31u) / 32u;   // 256 threads: 32 teams
    hipLaunchKernelGGL(k_tcp_build_bursts, dim3(g), dim3(256), 0, stream, dst, dst_len, src, src_len, hdrs, n_hdr, bursts,
                       n_bursts, frame_off, n_frames, frame_cap, frame_len_out, out, status);
    return hipGetLastError();
}

}  // namespace vpcsum
