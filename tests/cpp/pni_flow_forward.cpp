// The PNI Fastpath entries from plain C++ the way GpuCsumBatch downcalls them: flowtabCreate ->
// flowtabUpdate -> flowtabSetFastpath -> natFlowForwardFrames -> waitFor -> flowtabClose on a handful
// of frames of a registered arena.  tests/test_gpu_fastpath.py builds it like pni_flow.cpp and passes
// the bytes in a file: u32 arena_len, u32 flows, u32 frames, u32 Fastpath records, the arena, the
// frame offsets (u64), the frame lengths (u32), the flows (96 B each), the records' keys (40 B each),
// the records (16 B each), u32 keys of those not in the table, the expected arena, the expected
// status bytes, verdicts and ports (u32).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "vpcsum.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: pni_flow_forward vectors-file");
    FILE* f = fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    uint32_t hdr[4] = {0, 0, 0, 0};
    CHECK(fread(hdr, sizeof(hdr), 1, f) == 1, "header");
    const uint32_t len = hdr[0], nflows = hdr[1], n = hdr[2], nfp = hdr[3];
    CHECK(len > 0 && len < (1u << 20) && nflows > 0 && nflows < 16 && n > 0 && n <= 16 && nfp > 0 && nfp < 16, "header values");
    std::vector<uint8_t> in(len), want(len), want_st(n), want_vd(n);
    std::vector<vpcsum_flow_t> flows(nflows);
    std::vector<vpcsum_tuple_t> keys(nfp);
    std::vector<vpcsum_fastpath_t> fps(nfp);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> flen(n), want_port(n);
    uint32_t want_missing = 0;
    CHECK(fread(in.data(), 1, len, f) == len && fread(off.data(), 8, n, f) == n && fread(flen.data(), 4, n, f) == n &&
          fread(flows.data(), sizeof(vpcsum_flow_t), nflows, f) == nflows && fread(keys.data(), sizeof(vpcsum_tuple_t), nfp, f) == nfp &&
          fread(fps.data(), sizeof(vpcsum_fastpath_t), nfp, f) == nfp && fread(&want_missing, 4, 1, f) == 1 &&
          fread(want.data(), 1, len, f) == len && fread(want_st.data(), 1, n, f) == n && fread(want_vd.data(), 1, n, f) == n &&
          fread(want_port.data(), 4, n, f) == n, "short file");
    fclose(f);

    PNIEnv_vpcsum_long envl;
    PNIEnv_vpcsum_void envv;
    PNIEnv_vpcsum_int envi;
    memset(&envl, 0, sizeof(envl));
    memset(&envv, 0, sizeof(envv));
    memset(&envi, 0, sizeof(envi));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_create(&envl, 0, 1 << 20, 64) == 0, "pni create");
    const int64_t h = envl.return_;
    memset(&envl, 0, sizeof(envl));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabCreate(&envl, 0, 16) == 0, "pni flowtabCreate: %s", vpcsum_last_error());
    const int64_t tab = envl.return_;
    CHECK(tab != 0, "flowtabCreate returned 0");
    std::vector<uint8_t> reg(in);
    CHECK(Java_io_vproxy_vpcsum_VPCsum_registerArena(&envv, h, reg.data(), (int64_t)len) == 0, "pni register");
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate(&envv, tab, nullptr, 0, flows.data(), (int32_t)nflows) == 0,
          "pni flowtabUpdate: %s", vpcsum_last_error());
    // a malformed key throws and changes nothing; a negative count throws
    vpcsum_tuple_t bad = keys[0];
    bad.l3_ver = 5;
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(&envi, tab, &bad, fps.data(), 1) == -1 && envi.ex.type != nullptr,
          "a malformed key must throw");
    memset(&envi, 0, sizeof(envi));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(&envi, tab, keys.data(), fps.data(), -1) == -1 && envi.ex.type != nullptr,
          "a negative count must throw");
    memset(&envi, 0, sizeof(envi));
    envi.return_ = -5;
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(&envi, tab, keys.data(), fps.data(), (int32_t)nfp) == 0,
          "pni flowtabSetFastpath: %s", vpcsum_last_error());
    CHECK(envi.return_ == (int32_t)want_missing, "flowtabSetFastpath: %d keys missing, expected %u", envi.return_, want_missing);

    for (int mode : {VPCSUM_NAT_RFC1624, VPCSUM_NAT_STRICT_JAVA}) {
        memcpy(reg.data(), in.data(), len);
        std::vector<uint8_t> st(n, 0xee), vd(n, 0xee);
        std::vector<uint32_t> port(n, 0xeeeeeeeeu);
        memset(&envl, 0, sizeof(envl));
        CHECK(Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames(&envl, h, tab, reg.data(), (int64_t)len, off.data(), flen.data(),
                                                                (int32_t)n, st.data(), vd.data(), port.data(), mode) == 0,
              "pni natFlowForwardFrames mode %d: %s", mode, vpcsum_last_error());
        CHECK(Java_io_vproxy_vpcsum_VPCsum_waitFor(&envv, h, envl.return_) == 0, "wait");
        for (uint32_t i = 0; i < n; ++i) {
            CHECK(vd[i] == want_vd[i], "mode %d: frame %u verdict %u, expected %u", mode, i, vd[i], want_vd[i]);
            CHECK(st[i] == want_st[i], "mode %d: frame %u status %02x, expected %02x", mode, i, st[i], want_st[i]);
            CHECK(port[i] == want_port[i], "mode %d: frame %u port %u, expected %u", mode, i, port[i], want_port[i]);
        }
        for (uint32_t k = 0; k < len; ++k)
            CHECK(reg[k] == want[k], "mode %d: byte %u is %02x, expected %02x", mode, k, reg[k], want[k]);
    }
    // a NULL port array and an unregistered arena throw
    std::vector<uint8_t> st(n), vd(n);
    std::vector<uint32_t> port(n);
    memset(&envl, 0, sizeof(envl));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames(&envl, h, tab, reg.data(), (int64_t)len, off.data(), flen.data(),
                                                            (int32_t)n, st.data(), vd.data(), nullptr, 0) == -1 &&
              envl.ex.type != nullptr,
          "a NULL port array must throw");
    std::vector<uint8_t> pageable(in);
    memset(&envl, 0, sizeof(envl));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames(&envl, h, tab, pageable.data(), (int64_t)len, off.data(), flen.data(),
                                                            (int32_t)n, st.data(), vd.data(), port.data(), 0) == -1 &&
              envl.ex.type != nullptr,
          "an unregistered arena must throw");
    Java_io_vproxy_vpcsum_VPCsum_close(&envv, h);
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabClose(&envv, tab) == 0, "pni flowtabClose");
    printf("pni flow forward ok\n");
    return 0;
}
