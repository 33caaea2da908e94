// The PNI NAT entry (VPCsum.natSubmit) with VPCSUM_NAT_TCP_REWRITES, from plain C++ the way
// GpuCsumBatch downcalls it: three frames -- an MSS clamp, a SYN without the option (S_MSS_ABSENT)
// and a PROXY-protocol SYN-ACK build -- in both modes, zero-copy (registered arena) and staged.
// tests/test_gpu_tcprw.py builds it like capi_smoke and passes the bytes in a file: u32 arena_len,
// the arena, 3 descriptors, 3 entries, the expected arena, 3 expected status bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "vpcsum.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: pni_nat_tcp vectors-file");
    FILE* f = fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    uint32_t len = 0;
    CHECK(fread(&len, 4, 1, f) == 1 && len > 0 && len < (1u << 20), "arena length");
    std::vector<uint8_t> in(len), want(len);
    vpcsum_desc_t d[3];
    vpcsum_nat_t rw[3];
    uint8_t want_st[3];
    CHECK(fread(in.data(), 1, len, f) == len && fread(d, sizeof(d), 1, f) == 1 && fread(rw, sizeof(rw), 1, f) == 1 &&
          fread(want.data(), 1, len, f) == len && fread(want_st, 1, 3, f) == 3, "short file");
    fclose(f);

    PNIEnv_vpcsum_long envl;
    PNIEnv_vpcsum_void envv;
    memset(&envl, 0, sizeof(envl));
    memset(&envv, 0, sizeof(envv));
    CHECK(Java_io_vproxy_vpcsum_VPCsum_create(&envl, 0, 1 << 20, 64) == 0, "pni create");
    const int64_t h = envl.return_;
    std::vector<uint8_t> reg(len), pageable(len);
    CHECK(Java_io_vproxy_vpcsum_VPCsum_registerArena(&envv, h, reg.data(), (int64_t)len) == 0, "pni register");
    for (int mode : {VPCSUM_NAT_RFC1624 | VPCSUM_NAT_TCP_REWRITES, VPCSUM_NAT_STRICT_JAVA | VPCSUM_NAT_TCP_REWRITES}) {
        for (int staged = 0; staged < 2; ++staged) {
            uint8_t* a = staged ? pageable.data() : reg.data();
            memcpy(a, in.data(), len);
            uint8_t st[3] = {0, 0, 0};
            memset(&envl, 0, sizeof(envl));
            CHECK(Java_io_vproxy_vpcsum_VPCsum_natSubmit(&envl, h, a, (int64_t)len, d, rw, 3, st, mode) == 0,
                  "pni natSubmit mode %d: %s", mode, vpcsum_last_error());
            CHECK(Java_io_vproxy_vpcsum_VPCsum_waitFor(&envv, h, envl.return_) == 0, "nat wait");
            CHECK(memcmp(st, want_st, 3) == 0, "mode %d staged %d: status %02x %02x %02x, expected %02x %02x %02x", mode, staged,
                  st[0], st[1], st[2], want_st[0], want_st[1], want_st[2]);
            for (uint32_t k = 0; k < len; ++k)
                CHECK(a[k] == want[k], "mode %d staged %d: byte %u is %02x, expected %02x", mode, staged, k, a[k], want[k]);
        }
    }
    // the mode bit alone is what a caller probes; a bit beyond it is still refused, with a message
    memset(&envl, 0, sizeof(envl));
    uint8_t st[3];
    CHECK(Java_io_vproxy_vpcsum_VPCsum_natSubmit(&envl, h, reg.data(), (int64_t)len, d, rw, 3, st, 4) == -1, "mode 4 must throw");
    CHECK(envl.ex.type != nullptr, "exception type");
    Java_io_vproxy_vpcsum_VPCsum_close(&envv, h);
    printf("pni nat tcp ok\n");
    return 0;
}
