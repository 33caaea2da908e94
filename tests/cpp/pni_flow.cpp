// The PNI flow-table entries from plain C++ the way GpuCsumBatch downcalls them: flowtabCreate ->
// flowtabUpdate -> natFlowFrames -> waitFor -> flowtabCollect -> flowtabClose on three frames of a
// registered arena -- a hit, a punt (the flow's SYN) and a miss.  tests/test_gpu_flow.py builds it
// like pni_nat_tcp.cpp and passes the bytes in a file: u32 arena_len, u32 flows, the arena, 3 frame
// offsets (u64), 3 frame lengths (u32), the flows (96 B each), the expected arena, 3 expected status
// bytes, 3 expected verdicts, the cookie collect must return.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "vpcsum.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: pni_flow vectors-file");
    FILE* f = fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    uint32_t len = 0, nflows = 0;
    CHECK(fread(&len, 4, 1, f) == 1 && fread(&nflows, 4, 1, f) == 1 && len > 0 && len < (1u << 20) && nflows > 0 && nflows < 16,
          "header");
    std::vector<uint8_t> in(len), want(len);
    std::vector<vpcsum_flow_t> flows(nflows);
    uint64_t off[3];
    uint32_t flen[3];
    uint8_t want_st[3], want_vd[3];
    uint64_t want_cookie = 0;
    CHECK(fread(in.data(), 1, len, f) == len && fread(off, sizeof(off), 1, f) == 1 && fread(flen, sizeof(flen), 1, f) == 1 &&
          fread(flows.data(), sizeof(vpcsum_flow_t), nflows, f) == nflows && fread(want.data(), 1, len, f) == len &&
          fread(want_st, 1, 3, f) == 3 && fread(want_vd, 1, 3, f) == 3 && fread(&want_cookie, 8, 1, f) == 1, "short file");
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
    // a malformed flow throws and changes nothing
    vpcsum_flow_t bad = flows[0];
    bad.key.l4_proto = 1;
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate(&envv, tab, nullptr, 0, &bad, 1) == -1 && envv.ex.type != nullptr,
          "a malformed flow must throw");
    memset(&envv, 0, sizeof(envv));

    for (int mode : {VPCSUM_NAT_RFC1624, VPCSUM_NAT_STRICT_JAVA}) {
        memcpy(reg.data(), in.data(), len);
        uint8_t st[3] = {0xee, 0xee, 0xee}, vd[3] = {0xee, 0xee, 0xee};
        memset(&envl, 0, sizeof(envl));
        CHECK(Java_io_vproxy_vpcsum_VPCsum_natFlowFrames(&envl, h, tab, reg.data(), (int64_t)len, off, flen, 3, st, vd, mode) == 0,
              "pni natFlowFrames mode %d: %s", mode, vpcsum_last_error());
        CHECK(Java_io_vproxy_vpcsum_VPCsum_waitFor(&envv, h, envl.return_) == 0, "wait");
        CHECK(memcmp(vd, want_vd, 3) == 0, "mode %d: verdicts %u %u %u, expected %u %u %u", mode, vd[0], vd[1], vd[2], want_vd[0],
              want_vd[1], want_vd[2]);
        CHECK(memcmp(st, want_st, 3) == 0, "mode %d: status %02x %02x %02x, expected %02x %02x %02x", mode, st[0], st[1], st[2],
              want_st[0], want_st[1], want_st[2]);
        for (uint32_t k = 0; k < len; ++k)
            CHECK(reg[k] == want[k], "mode %d: byte %u is %02x, expected %02x", mode, k, reg[k], want[k]);
        uint64_t cookies[4] = {0, 0, 0, 0};
        CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabCollect(&envi, tab, cookies, 4) == 0, "pni flowtabCollect: %s", vpcsum_last_error());
        CHECK(envi.return_ == 1 && cookies[0] == want_cookie, "collect: %d flows, first cookie %llx, expected 1 and %llx", envi.return_,
              (unsigned long long)cookies[0], (unsigned long long)want_cookie);
        CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabCollect(&envi, tab, cookies, 4) == 0 && envi.return_ == 0, "second collect");
    }
    // an unregistered arena throws
    std::vector<uint8_t> pageable(in);
    uint8_t st[3], vd[3];
    memset(&envl, 0, sizeof(envl));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_natFlowFrames(&envl, h, tab, pageable.data(), (int64_t)len, off, flen, 3, st, vd, 0) == -1 &&
              envl.ex.type != nullptr,
          "an unregistered arena must throw");
    Java_io_vproxy_vpcsum_VPCsum_close(&envv, h);
    CHECK(Java_io_vproxy_vpcsum_VPCsum_flowtabClose(&envv, tab) == 0, "pni flowtabClose");
    printf("pni flow ok\n");
    return 0;
}
