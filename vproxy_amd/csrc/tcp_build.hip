// tcp_build.hip -- k_tcp_build (vpcsum_tcp_build_async): finished TCP data segments from "connection
// header + payload run".  Per record, the payload is read once from the send buffer, written once
// into the frame and added to the segment's one's complement accumulator between the two; the
// headers are generated in registers from the 64-B template and stored, with both sums, after the
// team's reduction.  No second kernel, no re-read of the written frame.
//
// A team of 8 lanes per record (K2's shape for frames) loads the record and runs tcp_frame.h's body,
// which k_tcp_build_bursts (tcp_burst.hip) runs too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "internal.h"
#include "tcp_frame.h"

namespace vpcsum {

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
    const u32x4a4_t ra = *(gu32x4a4_t*)(segs + i);
    const u32x4a4_t rb = *(gu32x4a4_t*)((const uint8_t*)(segs + i) + 16);
    const uint64_t frame_off = ((uint64_t)ra.y << 32) | ra.x, data_off = ((uint64_t)ra.w << 32) | ra.z;
    const uint32_t seq = rb.x, hdr = rb.y, frame_cap = rb.z;
    const uint32_t data_len = rb.w & 0xffffu, flags = (rb.w >> 16) & 0xffu, rsv = rb.w >> 24;

    tcp_build_frame(dst, dst_len, src, src_len, hdrs, n_hdr, i, tl, frame_off, data_off, seq, hdr, frame_cap, data_len, flags,
                    rsv, frame_len_out, out, status, [](const uint32_t (&)[16]) { return true; });
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
