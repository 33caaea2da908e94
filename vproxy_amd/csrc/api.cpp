// api.cpp -- the C-ABI of libvpcsum.so (declared in include/vpcsum.h).
//
// Device-resident entry points validate arguments and launch the kernels of kernels.hip on
// the caller's stream.  The context API is what the Java side drives (io.vproxy.vpcsum.VPCsum,
// java/io/vproxy/vpcsum/VPCsum.java): host arena + descriptors in, checksums out, with the
// batch flushed once per Iface.completeTx (core/.../vswitch/iface/XDPIface.java:227-243).
// Errors: plain functions return <0 and set a thread-local message; PNI functions store the
// exception in env->ex exactly as the PNI runtime expects (base/src/main/c-generated/pni.h:74-82).
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "batch_plan.h"
#include "flow_table.h"
#include "internal.h"
#include "tcp_build.h"
#include "tcp_burst.h"
#include "tcp_recv.h"
#include "icmp_reply.h"
#include "udp_build.h"
#include "udp_recv.h"
#include "vpcsum.h"

namespace vpcsum {

// The thread's last error message: a fixed buffer, so that reporting a failure never allocates
// (an out-of-memory failure must still leave its message)
static thread_local char g_err[1024];

static int fail(const char* fmt, ...) {
    char buf[sizeof(g_err)];   // the arguments may point into g_err itself
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    memcpy(g_err, buf, sizeof(g_err));
    return -1;
}

static int hipfail(hipError_t e, const char* what) {
    return fail("%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

// Every extern "C" entry point catches what the C++ runtime may throw (std::bad_alloc from the
// bookkeeping containers, ...): an exception must never unwind into a C or JVM caller.  The entry
// returns -1 with the message set (PNI: the exception stored in env->ex).
#define VPC_CATCH(what)                                                                 \
    catch (const std::bad_alloc&) { return fail("%s: out of host memory", what); }     \
    catch (...) { return fail("%s: internal error (C++ exception)", what); }
#define VPC_CATCH_PNI(what)                                                             \
    catch (const std::bad_alloc&) {                                                     \
        fail("%s: out of host memory", what);                                           \
        return pni_throw(env, "java.lang.OutOfMemoryError");                            \
    }                                                                                   \
    catch (...) {                                                                       \
        fail("%s: internal error (C++ exception)", what);                               \
        return pni_throw(env, "java.io.IOException");                                   \
    }

#define VPC_CHECK(expr, what)                         \
    do {                                              \
        hipError_t e__ = (expr);                      \
        if (e__ != hipSuccess) return hipfail(e__, what); \
    } while (0)

// Makes `device` current for one entry point and gives the caller its own current device back on
// every exit path: a torch or Java caller working on another device never sees it change.
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

#define VPC_ON_DEVICE(dev)                                                      \
    DeviceScope dscope__(dev);                                                  \
    if (dscope__.err != hipSuccess) return hipfail(dscope__.err, "hipSetDevice")

int num_cus(int device) {
    static std::mutex mu;
    static std::vector<int> cache;
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0) device = 0;
    if ((int)cache.size() <= device) cache.resize(device + 1, 0);
    if (cache[device] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 256;
        cache[device] = v;
    }
    return cache[device];
}

// A buffer that frees itself: Free releases the host pointer p.  Move-only, so that assigning a
// fresh Slot or Service over a used one frees what the old one held, member by member.
template <class T, hipError_t (*Free)(void*)>
struct Owned {
    T* p = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : p(o.p) { o.p = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        free();   // (a buffer moved onto itself ends up empty)
        p = o.p;
        o.p = nullptr;
        return *this;
    }
    ~Owned() { free(); }
    void free() {
        if (p) (void)Free(p);
        p = nullptr;
    }
};

// A pinned host buffer the device reads and writes in place (mapped, coherent: uncached on the
// GPU): the host pointer and its device address as one value.  alloc() pins and maps; the context
// and the service pin a group of buffers before they map them, with pin() and map().
template <class T>
struct Mapped : Owned<T, hipHostFree> {
    T* dev = nullptr;   // the same bytes as the device addresses them (valid while p is)
    hipError_t pin(size_t bytes) { return hipHostMalloc((void**)&this->p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
    hipError_t map() { return hipHostGetDevicePointer((void**)&dev, this->p, 0); }
    hipError_t alloc(size_t bytes) {
        hipError_t e = pin(bytes);
        if (e == hipSuccess) e = map();
        if (e != hipSuccess) this->free();
        return e;
    }
};

// Its device-only twin: device memory no host code addresses.
template <class T>
struct DeviceOnly : Owned<T, hipFree> {
    hipError_t alloc(size_t bytes) { return hipMalloc((void**)&this->p, bytes); }
};

// One copy of a finished batch's results into a buffer of the caller's.
struct HandBack { void* dst; const void* src; size_t bytes; };
// The most any entry hands back: the status bytes and three more arrays (the ICMP replies: frame
// lengths, the replies' sums, the requests' verdict words)
constexpr size_t kHandBackMax = 4;

// What a staged batch scatters into the caller's frames when it is finished.
enum class Scatter { None, NatHeaders, CsumFields };

// The batch a slot owns from its submit to the wait (or the later submit) that finishes it.
struct Batch {
    Scatter scatter = Scatter::None;
    bool zero_copy = false;            // ran on the host frames in place
    uint32_t svc_seq = 0;              // != 0: went to the low-latency service (no event to wait for)
    uint64_t ticket = 0;
    uint32_t n = 0;
    uint32_t mode = 0;
    uint8_t* user_arena = nullptr;             // staged batch: the frames the scatter goes back into
    const vpcsum_desc_t* user_desc = nullptr;
    HandBack back[kHandBackMax] = {};          // the copies slot_finish makes, in this order
    uint32_t n_back = 0;
    // The entry lists its results once it knows where they will lie (the slot's staging or the
    // service's buffers).  A NULL destination -- the caller did not ask -- or an empty array is no copy.
    template <size_t N>
    void hand_back(const HandBack (&list)[N]) {
        static_assert(N <= kHandBackMax, "kHandBackMax: the largest entry's need");
        for (const HandBack& h : list)
            if (h.dst && h.bytes) back[n_back++] = h;
    }
};

// Per-slot staging of one in-flight batch of a context.
struct Slot {
    DeviceOnly<uint8_t> d_arena;
    DeviceOnly<vpcsum_desc_t> d_desc;
    DeviceOnly<uint32_t> d_out;
    DeviceOnly<uint8_t> d_status;
    Mapped<vpcsum_desc_t> h_desc;      // pinned staging
    Mapped<uint32_t> h_out;
    Mapped<uint8_t> h_status;
    Owned<uint8_t, hipHostFree> h_arena;   // pinned staging for unregistered arenas (not mapped)
    Mapped<uint64_t> h_foff;           // received-frame offsets / lengths
    Mapped<uint32_t> h_flen;
    // Per-packet scratch, max_pkts elements each, allocated by slot_scratch with the context's first
    // batch that needs it and freed, in this order, when a fresh Slot is assigned over this one:
    Mapped<vpcsum_nat_t> h_rw;         // per-packet entries (NAT rewrites, pre-images: at most 48 B each)
    DeviceOnly<vpcsum_nat_t> d_rw;     // and their device copy
    Mapped<vpcsum_tuple_t> h_tu;       // flow tuples of a parse batch
    Mapped<vpcsum_hsum_t> h_hs;        // ingress header sums of a verify batch
    DeviceOnly<vpcsum_tuple_t> d_tu;   // a flow batch's tuples (parse -> lookup)
    Mapped<uint8_t> h_verdict;         // and its verdicts
    DeviceOnly<vpcsum_fastpath_t> d_fp;   // a forwarding flow batch's Fastpath records (lookup -> L2 write)
    Mapped<uint32_t> h_port;           // and its output ports (an ICMP reply batch's d_csum words)
    Mapped<vpcsum_tcpseg_t> h_tseg;    // a TCP build batch's records (a UDP build batch's: the same 32 B; an ICMP reply batch's: 24 B), templates and frame lengths
    Mapped<vpcsum_tcphdr_t> h_thdr;
    Mapped<uint32_t> h_tlen;           // (a TCP receive batch's stored counts too)
    Mapped<vpcsum_tcprx_t> h_trx;      // a TCP receive batch's records (a UDP receive batch's: the same 16 B)
    Mapped<vpcsum_tcpburst_t> h_tburst;   // a TCP burst batch's records (its frame table: h_foff)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool busy = false;                 // `batch` is in flight
    Batch batch;
};

}  // namespace vpcsum

struct Registered {
    uint8_t* host;
    uint64_t len;
    uint8_t* dev;    // device-side address of the page-locked mapping (zero-copy access)
    uint8_t* key;    // the process-wide page-lock this entry holds a reference on (hostlock_acquire);
                     // nullptr: a mapping of its group's lock (the group holds the reference)
};

// ------------------------------------------------------------------------------------------
// Process-wide registry of the host ranges libvpcsum page-locks.  HIP keys a host registration by
// its start address (tools/reg_probe.py, profiles/r06c_reg_probe.jsonl): a second hipHostRegister
// of a registered start -- same length or longer -- returns success without mapping anything new,
// the first hipHostUnregister then drops the registration for both holders, and the second fails.
// Two contexts (or a context and a group) registering one umem therefore left the survivor with a
// mapping HIP had torn down, and its zero-copy kernels -- or a later pageable copy HIP resolves
// through the orphaned registration -- reading unmapped memory (DESIGN_HISTORY.md "Round 6: the
// intermittent fault").  So every page-lock goes through here: a range inside a live lock shares
// it (reference counted), a range that partially overlaps one or that HIP already holds as
// page-locked memory of another owner is refused, and hipHostUnregister runs once, with the last
// reference.  Locks are mapped on every device (portable), so a share across devices is valid.
// ------------------------------------------------------------------------------------------
struct HostLock {
    uint8_t* host;
    uint64_t len;
    uint32_t refs;
};
static std::mutex g_lock_mu;
static std::vector<HostLock> g_locks;

static bool hip_holds_pinned(const uint8_t* p) {
    hipPointerAttribute_t a;
    const bool pinned = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    (void)hipGetLastError();   // an unknown (pageable) pointer leaves an error behind
    return pinned;
}

using vpcsum::fail;
using vpcsum::hipfail;

// A reference on the page-lock of [p, p+len) (see HostLock): *key = the lock's start, for
// hostlock_release.  Caller is on the device the mapping is wanted for.
static int hostlock_acquire(uint8_t* p, uint64_t len, uint8_t** key, const char* what) {
    std::lock_guard<std::mutex> lk(g_lock_mu);
    for (auto& h : g_locks) {
        if (p >= h.host && p + len <= h.host + h.len) {   // inside a live lock: share it
            ++h.refs;
            *key = h.host;
            return 0;
        }
        if (p < h.host + h.len && h.host < p + len)
            return fail("%s: [%p, +%llu) overlaps the arena [%p, +%llu) page-locked earlier: register one range "
                        "that covers both",
                        what, (void*)p, (unsigned long long)len, (void*)h.host, (unsigned long long)h.len);
    }
    if (hip_holds_pinned(p) || hip_holds_pinned(p + len - 1))
        return fail("%s: %p is already page-locked outside libvpcsum (hipHostMalloc / hipHostRegister): its owner "
                    "controls that lock's lifetime; pass the memory unregistered (staged) instead",
                    what, (void*)p);
    g_locks.reserve(g_locks.size() + 1);   // may throw: before anything is pinned
    VPC_CHECK(hipHostRegister(p, len, hipHostRegisterMapped | hipHostRegisterPortable), "hipHostRegister");
    g_locks.push_back({p, len, 1});
    *key = p;
    return 0;
}

// Drop one reference; the last one unpins (a failure is reported: the caller must not free the
// memory as if it were unpinned).
static int hostlock_release(uint8_t* key, const char* what) {
    std::lock_guard<std::mutex> lk(g_lock_mu);
    for (size_t i = 0; i < g_locks.size(); ++i) {
        if (g_locks[i].host != key) continue;
        if (--g_locks[i].refs) return 0;
        g_locks.erase(g_locks.begin() + i);
        const hipError_t e = hipHostUnregister(key);
        if (e != hipSuccess) return fail("%s: hipHostUnregister(%p): %s", what, (void*)key, hipGetErrorString(e));
        return 0;
    }
    return fail("%s: %p holds no page-lock of libvpcsum", what, (void*)key);
}

// Zero-copy batches (frames read over PCIe) of at most this many packets run one wave per packet.
constexpr uint32_t kZeroCopyWaveTeams = 4096;
// kSvcBatchMax (internal.h): the largest batch handed to the low-latency service (128 waves, one
// packet each per round); larger ones are launched with a grid of their size, which is faster from
// ~1000 packets on (tools/flush_latency.cpp: 1024 packets 55 us launched vs 58 us through the
// service, profiles/r05m_flush_latency.json).

// The service's aux buffer: kSvcBatchMax pre-images of 48 B, or kSvcBatchMax descriptors followed
// by kSvcBatchMax tuples (a parse batch, kSvcParse)
constexpr size_t kSvcAuxBytes = (size_t)vpcsum::kSvcBatchMax * (sizeof(vpcsum_desc_t) + sizeof(vpcsum_tuple_t));
static_assert(kSvcAuxBytes >= (size_t)vpcsum::kSvcBatchMax * sizeof(vpcsum_pre_t), "aux buffer holds a batch of pre-images");

// Low-latency service of a context (kernels.hip k_csum_service).
struct Service {
    vpcsum::Mapped<vpcsum::SvcMailbox> mb;   // host-pinned, coherent (uncached on the GPU), mapped
    uint32_t* ctr = nullptr;             // device: workgroups finished with the current batch,
                                         // then (8-B aligned, ctr + 2) the command relay
    hipStream_t stream = nullptr;
    // the service's own descriptor / result buffers (pinned, coherent, mapped): the same for every
    // batch, so the parameter block rarely changes
    vpcsum::Mapped<vpcsum_desc_t> h_desc;
    vpcsum::Mapped<uint32_t> h_out;
    vpcsum::Mapped<uint8_t> h_status;
    vpcsum::Mapped<uint8_t> h_pre;       // the aux buffer (kSvcAuxBytes): pre-images of a batch with F_PRE
                                         // frames, or a parse batch's descriptors and tuples
    uint64_t par[3] = {0, 0, 0};         // arena, arena_len, arena_w last published
    bool par_valid = false;
    uint32_t posted = 0;                 // last batch published (seq)
    uint64_t idle_ticks = 0;             // 100 MHz ticks
    uint32_t grid = vpcsum::kServiceGrid;   // workgroups (VPCSUM_SVC_GRID: A/B tooling)
    uint32_t poll = 1;                      // relay poll mode: relaxed loads (VPCSUM_SVC_POLL: A/B tooling)
    bool on = false;
    bool inline_desc = true;             // descriptors of <= kSvcInlineDesc frames ride in the command line
                                         // (VPCSUM_SVC_INLINE=0 turns it off: A/B tooling)
#ifdef VPCSUM_SVC_STAMPS
    std::chrono::steady_clock::time_point t_post;
    uint32_t t_n = 0;
#endif
};

struct vpcsum_ctx {
    int device = 0;
    Service svc;
    uint64_t svc_batches = 0;    // batches run by the service (lifetime of the context)
    uint64_t svc_launches = 0;   // service grids launched (first start, idle restarts, re-runs)
    uint64_t max_arena = 0;
    uint32_t max_pkts = 0;
    vpcsum::Slot slots[2];
    uint64_t next_ticket = 1;
    std::vector<Registered> registered;
    std::mutex mu;
};

using namespace vpcsum;

extern "C" {

int vpcsum_abi_version(void) { return VPCSUM_ABI_VERSION; }

const char* vpcsum_last_error(void) { return g_err; }

int vpcsum_device_count(int* out_n) {
    try {
        if (!out_n) return fail("vpcsum_device_count: out_n is NULL");
        int n = 0;
        VPC_CHECK(hipGetDeviceCount(&n), "hipGetDeviceCount");
        *out_n = n;
        return 0;
    } VPC_CATCH("vpcsum_device_count")
}

int vpcsum_set_device(int device) {
    try {
        VPC_CHECK(hipSetDevice(device), "hipSetDevice");
        return 0;
    } VPC_CATCH("vpcsum_set_device")
}

int vpcsum_compute_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, uint32_t n,
                         uint32_t* d_out, uint8_t* d_status, uint32_t mode, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_desc) return fail("vpcsum_compute_async: NULL arena or descriptors");
        // beyond VERIFY and WRITE: tuning hints, not part of the stable ABI (launch_modes.h)
        if (mode & ~kCsumModeAccept) return fail("vpcsum_compute_async: bad mode 0x%x", mode);
        uint8_t* w = (mode & VPCSUM_MODE_WRITE) ? const_cast<uint8_t*>(d_arena) : nullptr;
        VPC_CHECK(launch_csum(d_arena, arena_len, d_desc, n, d_out, d_status, nullptr, (mode & VPCSUM_MODE_VERIFY) != 0, w,
                              csum_tune(mode), (hipStream_t)stream),
                  "vpcsum_compute_async launch");
        return 0;
    } VPC_CATCH("vpcsum_compute_async")
}

}  // extern "C"

// Two batches in flight on the device API (vpcsum.h vpcsum_pipe_*): launches alternate between two
// streams of the pipe's own, forked from the caller's stream at vpcsum_pipe_begin and joined back
// into it at vpcsum_pipe_join, so that one launch's ramp-up and drain overlap its neighbour's.
struct vpcsum_pipe {
    int device = 0;
    hipStream_t caller = nullptr;
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
    uint32_t next = 0;
};

static void pipe_free(vpcsum_pipe* p) {
    for (int i = 0; i < 2; ++i) {
        if (p->s[i]) {
            (void)hipStreamSynchronize(p->s[i]);
            (void)hipStreamDestroy(p->s[i]);
        }
        if (p->done[i]) (void)hipEventDestroy(p->done[i]);
    }
    if (p->fork) (void)hipEventDestroy(p->fork);
    delete p;
}

extern "C" {

int vpcsum_pipe_create(void* stream, vpcsum_pipe_t** out) {
    try {
        if (!out) return fail("vpcsum_pipe_create: out is NULL");
        vpcsum_pipe* p = new vpcsum_pipe();
        p->caller = (hipStream_t)stream;
        hipError_t e = hipGetDevice(&p->device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->s[0], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->s[1], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done[0], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done[1], hipEventDisableTiming);
        if (e != hipSuccess) {
            pipe_free(p);
            return hipfail(e, "vpcsum_pipe_create");
        }
        *out = p;
        return 0;
    } VPC_CATCH("vpcsum_pipe_create")
}

int vpcsum_pipe_begin(vpcsum_pipe_t* p) {
    try {
        if (!p) return fail("vpcsum_pipe_begin: NULL pipe");
        VPC_ON_DEVICE(p->device);
        VPC_CHECK(hipEventRecord(p->fork, p->caller), "vpcsum_pipe_begin: hipEventRecord");
        for (int i = 0; i < 2; ++i) VPC_CHECK(hipStreamWaitEvent(p->s[i], p->fork, 0), "vpcsum_pipe_begin: hipStreamWaitEvent");
        return 0;
    } VPC_CATCH("vpcsum_pipe_begin")
}

int vpcsum_pipe_compute_async(vpcsum_pipe_t* p, const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                              uint32_t n, uint32_t* d_out, uint8_t* d_status, uint32_t mode) {
    try {
        if (!p) return fail("vpcsum_pipe_compute_async: NULL pipe");
        VPC_ON_DEVICE(p->device);
        const int rc = vpcsum_compute_async(d_arena, arena_len, d_desc, n, d_out, d_status, mode, p->s[p->next & 1]);
        if (rc == 0) ++p->next;
        return rc;
    } VPC_CATCH("vpcsum_pipe_compute_async")
}

int vpcsum_pipe_join(vpcsum_pipe_t* p) {
    try {
        if (!p) return fail("vpcsum_pipe_join: NULL pipe");
        VPC_ON_DEVICE(p->device);
        for (int i = 0; i < 2; ++i) {
            VPC_CHECK(hipEventRecord(p->done[i], p->s[i]), "vpcsum_pipe_join: hipEventRecord");
            VPC_CHECK(hipStreamWaitEvent(p->caller, p->done[i], 0), "vpcsum_pipe_join: hipStreamWaitEvent");
        }
        return 0;
    } VPC_CATCH("vpcsum_pipe_join")
}

int vpcsum_pipe_destroy(vpcsum_pipe_t* p) {
    try {
        if (!p) return 0;
        DeviceScope on_dev(p->device);
        pipe_free(p);
        return 0;
    } VPC_CATCH("vpcsum_pipe_destroy")
}

// NAT on device memory: the rewrite kernel, then (strict Java) the full recompute of the sums it
// dirtied, written in place -- Java's getRawPacket(0) after the setters.
static int nat_run(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const void* d_rw, int fmt,
                   uint32_t n, uint8_t* d_status, uint32_t nat_mode, hipStream_t s) {
    // VPCSUM_NAT_TCP_REWRITES (48-B entries, a status buffer: the callers' checks): the TCP-header
    // rewrites of VPCSUM_NAT_TCP entries, a pass of their own after the rewrite
    const bool tcp = (nat_mode & VPCSUM_NAT_TCP_REWRITES) != 0;
    const NatBuild build = nat_build(nat_mode, fmt);
    if (nat_mode & VPCSUM_NAT_STRICT_JAVA) {
        // pass 1: rewrite fields, record which sums went dirty (Java's checksumSkipped())
        VPC_CHECK(launch_nat(d_arena, arena_len, d_desc, d_rw, n, nullptr, d_status, build, s), "nat launch");
        if (tcp) VPC_CHECK(launch_nat_tcp(d_arena, arena_len, d_desc, d_rw, n, d_status, 1, s), "nat tcp launch");
        // pass 2: full recompute of the dirty sums, written in place (getRawPacket(0))
        VPC_CHECK(launch_csum(d_arena, arena_len, d_desc, n, nullptr, d_status, d_status, false, d_arena, CsumTune{}, s),
                  "nat recompute launch");
        // pass 3: the TTL-expired packets (refused, untouched) get S_TTL_EXPIRED next to S_BAD_DESC
        VPC_CHECK(launch_nat_ttl_status(d_arena, arena_len, d_desc, d_rw, fmt, n, d_status, s), "nat ttl status launch");
        // and the SYNs a clamp found without an MSS option S_MSS_ABSENT next to S_DONE
        if (tcp) VPC_CHECK(launch_nat_tcp(d_arena, arena_len, d_desc, d_rw, n, d_status, 2, s), "nat tcp status launch");
        return 0;
    }
    VPC_CHECK(launch_nat(d_arena, arena_len, d_desc, d_rw, n, d_status, nullptr, build, s), "nat launch");
    if (tcp) VPC_CHECK(launch_nat_tcp(d_arena, arena_len, d_desc, d_rw, n, d_status, 0, s), "nat tcp launch");
    return 0;
}

static int nat_async(const char* what, uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                     const void* d_rw, int fmt, uint32_t n, uint8_t* d_status, uint32_t nat_mode, void* stream) {
    if (n == 0) return 0;
    if (!d_arena || !d_desc || !d_rw) return fail("%s: NULL arena, descriptors or rewrite table", what);
    // beyond the two mode bits: tuning hints, not part of the stable ABI (launch_modes.h)
    if (nat_mode & ~kNatModeAccept)
        return fail("%s: bad nat_mode 0x%x", what, nat_mode);
    if ((nat_mode & VPCSUM_NAT_TCP_REWRITES) && fmt != 1)
        return fail("%s: VPCSUM_NAT_TCP_REWRITES takes 48-byte vpcsum_nat_t entries only (vpcsum_nat_async)", what);
    if ((nat_mode & VPCSUM_NAT_TCP_REWRITES) && !d_status) return fail("%s: VPCSUM_NAT_TCP_REWRITES needs a status buffer", what);
    if ((nat_mode & VPCSUM_NAT_STRICT_JAVA) && !d_status) return fail("%s: strict-java mode needs a status buffer", what);
    if ((nat_mode & VPCSUM_NAT_STRICT_JAVA) && fmt == 2) return fail("%s: records take VPCSUM_NAT_RFC1624 only", what);
    return nat_run(d_arena, arena_len, d_desc, d_rw, fmt, n, d_status, nat_mode, (hipStream_t)stream);
}

// tooling: the pattern probes take the tuning fields of a nat_mode word from the environment
static uint32_t nat_probe_tune() {
    static const uint32_t tune = [] {
        const char* e = getenv("VPCSUM_NAT_PROBE_TUNE");
        return e ? (uint32_t)strtoul(e, nullptr, 0) : 0u;
    }();
    return tune;
}

int vpcsum_nat4_pattern_probe_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                                    const vpcsum_nat4_t* d_rw, uint32_t n, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_desc || !d_rw) return fail("vpcsum_nat4_pattern_probe_async: NULL argument");
        VPC_CHECK(launch_nat(d_arena, arena_len, d_desc, d_rw, n, nullptr, nullptr, nat_probe_build(nat_probe_tune(), 0),
                             (hipStream_t)stream),
                  "vpcsum_nat4_pattern_probe_async launch");
        return 0;
    } VPC_CATCH("vpcsum_nat4_pattern_probe_async")
}

int vpcsum_nat4_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const vpcsum_nat4_t* d_rw,
                      uint32_t n, uint8_t* d_status, uint32_t nat_mode, void* stream) {
    try {
        return nat_async("vpcsum_nat4_async", d_arena, arena_len, d_desc, d_rw, 0, n, d_status, nat_mode, stream);
    } VPC_CATCH("vpcsum_nat4_async")
}

int vpcsum_nat4r_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_nat4_rec_t* d_rec, uint32_t n,
                       uint8_t* d_status, uint32_t nat_mode, void* stream) {
    try {
        return nat_async("vpcsum_nat4r_async", d_arena, arena_len, (const vpcsum_desc_t*)d_rec, d_rec, 2, n, d_status,
                         nat_mode, stream);
    } VPC_CATCH("vpcsum_nat4r_async")
}

int vpcsum_nat4r_pattern_probe_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_nat4_rec_t* d_rec,
                                     uint32_t n, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_rec) return fail("vpcsum_nat4r_pattern_probe_async: NULL argument");
        VPC_CHECK(launch_nat(d_arena, arena_len, (const vpcsum_desc_t*)d_rec, d_rec, n, nullptr, nullptr,
                             nat_probe_build(nat_probe_tune(), 2), (hipStream_t)stream),
                  "vpcsum_nat4r_pattern_probe_async launch");
        return 0;
    } VPC_CATCH("vpcsum_nat4r_pattern_probe_async")
}

int vpcsum_nat_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const vpcsum_nat_t* d_rw,
                     uint32_t n, uint8_t* d_status, uint32_t nat_mode, void* stream) {
    try {
        return nat_async("vpcsum_nat_async", d_arena, arena_len, d_desc, d_rw, 1, n, d_status, nat_mode, stream);
    } VPC_CATCH("vpcsum_nat_async")
}

int vpcsum_pre_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const void* d_pre,
                     uint32_t pre_fmt, uint32_t n, uint32_t* d_out, uint8_t* d_status, uint32_t mode, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_desc || !d_pre) return fail("vpcsum_pre_async: NULL arena, descriptors or pre-images");
        if (pre_fmt > VPCSUM_PRE_FMT_PRE) return fail("vpcsum_pre_async: bad pre_fmt %u", pre_fmt);
        // beyond WRITE: tuning hints, not part of the stable ABI (launch_modes.h)
        if (mode & ~kPreModeAccept) return fail("vpcsum_pre_async: bad mode 0x%x", mode);
        VPC_CHECK(launch_pre(d_arena, arena_len, d_desc, d_pre, n, d_out, d_status, pre_build(mode, (int)pre_fmt),
                             (hipStream_t)stream),
                  "vpcsum_pre_async launch");
        return 0;
    } VPC_CATCH("vpcsum_pre_async")
}

int vpcsum_parse_ether_async(const uint8_t* d_arena, uint64_t arena_len, const uint64_t* d_frame_off,
                             const uint32_t* d_frame_len, uint32_t n, uint8_t flags, vpcsum_desc_t* d_desc,
                             uint8_t* d_status, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_frame_off || !d_frame_len || !d_desc) return fail("vpcsum_parse_ether_async: NULL argument");
        VPC_CHECK(launch_parse_ether(d_arena, arena_len, d_frame_off, d_frame_len, n, flags, d_desc, d_status, nullptr,
                                     (hipStream_t)stream),
                  "parse launch");
        return 0;
    } VPC_CATCH("vpcsum_parse_ether_async")
}

int vpcsum_parse_ether_tuples_async(const uint8_t* d_arena, uint64_t arena_len, const uint64_t* d_frame_off,
                                    const uint32_t* d_frame_len, uint32_t n, uint8_t flags, vpcsum_desc_t* d_desc,
                                    uint8_t* d_status, vpcsum_tuple_t* d_tuples, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_frame_off || !d_frame_len || !d_desc || !d_tuples)
            return fail("vpcsum_parse_ether_tuples_async: NULL argument");
        if ((uintptr_t)d_tuples & 3) return fail("vpcsum_parse_ether_tuples_async: tuples not 4-byte aligned");
        VPC_CHECK(launch_parse_ether(d_arena, arena_len, d_frame_off, d_frame_len, n, flags, d_desc, d_status, d_tuples,
                                     (hipStream_t)stream),
                  "parse launch");
        return 0;
    } VPC_CATCH("vpcsum_parse_ether_tuples_async")
}

int vpcsum_parse_ether_hsum_async(const uint8_t* d_arena, uint64_t arena_len, const uint64_t* d_frame_off,
                                  const uint32_t* d_frame_len, uint32_t n, uint8_t flags, vpcsum_desc_t* d_desc,
                                  uint8_t* d_status, vpcsum_hsum_t* d_hsum, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_frame_off || !d_frame_len || !d_desc || !d_hsum)
            return fail("vpcsum_parse_ether_hsum_async: NULL argument");
        if ((uintptr_t)d_hsum & 7) return fail("vpcsum_parse_ether_hsum_async: header sums not 8-byte aligned");
        VPC_CHECK(launch_parse_ether(d_arena, arena_len, d_frame_off, d_frame_len, n, flags, d_desc, d_status, nullptr,
                                     (hipStream_t)stream, nullptr, d_hsum),
                  "parse launch");
        return 0;
    } VPC_CATCH("vpcsum_parse_ether_hsum_async")
}

int vpcsum_read_probe_async(const uint8_t* d_buf, uint64_t bytes, uint32_t* d_sink, uint32_t grid, void* stream) {
    try {
        if (!d_buf || !d_sink) return fail("vpcsum_read_probe_async: NULL argument");
        VPC_CHECK(launch_read_probe(d_buf, bytes, d_sink, grid, (hipStream_t)stream), "read probe launch");
        return 0;
    } VPC_CATCH("vpcsum_read_probe_async")
}

int vpcsum_pattern_probe_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, uint32_t n,
                               uint32_t* d_sink, uint32_t grid, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_desc || !d_sink) return fail("vpcsum_pattern_probe_async: NULL argument");
        if (arena_len >= (1ull << 32)) return fail("vpcsum_pattern_probe_async: arena must be < 4 GiB");
        VPC_CHECK(launch_pattern_probe(d_arena, arena_len, d_desc, n, d_sink, grid, (hipStream_t)stream),
                  "pattern probe launch");
        return 0;
    } VPC_CATCH("vpcsum_pattern_probe_async")
}

int vpcsum_synth_async(uint8_t* d_arena, uint64_t arena_len, uint32_t n, uint32_t stride, uint32_t l3_pad,
                       uint32_t workload, uint64_t seed, uint64_t first_index, vpcsum_desc_t* d_desc, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena && !d_desc) return fail("vpcsum_synth_async: NULL arena and descriptors");
        if (workload < VPCSUM_SYNTH_C1_UDP64 || workload > VPCSUM_SYNTH_C5_NAT1500) return fail("vpcsum_synth_async: bad workload %u", workload);
        const uint32_t maxlen = (workload == VPCSUM_SYNTH_C4_V6JUMBO || workload == VPCSUM_SYNTH_FUZZ) ? 9000
                                : (workload == VPCSUM_SYNTH_C1_UDP64) ? 50 : 1500;
        if ((uint64_t)l3_pad + maxlen > stride) return fail("vpcsum_synth_async: stride %u < l3_pad %u + %u", stride, l3_pad, maxlen);
        if (d_arena && (uint64_t)n * stride > arena_len) return fail("vpcsum_synth_async: arena too small");
        VPC_CHECK(launch_synth(d_arena, arena_len, n, stride, l3_pad, workload, seed, first_index, d_desc,
                               (hipStream_t)stream),
                  "synth launch");
        return 0;
    } VPC_CATCH("vpcsum_synth_async")
}

int vpcsum_spin_probe_async(uint32_t workgroups, uint32_t threads, uint32_t micros, void* stream) {
    try {
        if (workgroups == 0 || workgroups > 65535 || threads == 0 || threads > 1024 || (threads & 63))
            return fail("vpcsum_spin_probe_async: bad shape %u x %u", workgroups, threads);
        VPC_CHECK(launch_spin_probe(workgroups, threads, (uint64_t)micros * 100u, (hipStream_t)stream), "spin probe launch");
        return 0;
    } VPC_CATCH("vpcsum_spin_probe_async")
}

int vpcsum_event_create(void** ev) {
    try {
        if (!ev) return fail("vpcsum_event_create: NULL");
        hipEvent_t e;
        VPC_CHECK(hipEventCreate(&e), "hipEventCreate");
        *ev = (void*)e;
        return 0;
    } VPC_CATCH("vpcsum_event_create")
}
int vpcsum_event_destroy(void* ev) {
    try {
        VPC_CHECK(hipEventDestroy((hipEvent_t)ev), "hipEventDestroy");
        return 0;
    } VPC_CATCH("vpcsum_event_destroy")
}
int vpcsum_event_record(void* ev, void* stream) {
    try {
        VPC_CHECK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream), "hipEventRecord");
        return 0;
    } VPC_CATCH("vpcsum_event_record")
}
int vpcsum_event_elapsed_ms(void* start, void* end, float* ms) {
    try {
        if (!ms) return fail("vpcsum_event_elapsed_ms: NULL");
        VPC_CHECK(hipEventSynchronize((hipEvent_t)end), "hipEventSynchronize");
        VPC_CHECK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end), "hipEventElapsedTime");
        return 0;
    } VPC_CATCH("vpcsum_event_elapsed_ms")
}
int vpcsum_stream_sync(void* stream) {
    try {
        VPC_CHECK(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
        return 0;
    } VPC_CATCH("vpcsum_stream_sync")
}

// ------------------------------------------------------------------------------------------
// Context (host memory) API
// ------------------------------------------------------------------------------------------
static void slot_free(Slot& s) {
    const hipEvent_t done = s.done;
    const hipStream_t stream = s.stream;
    s = Slot();   // every buffer frees itself, in the order of its declaration, whatever members there are
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
}

static int slot_finish(vpcsum_ctx* c, Slot& s);

static void svc_free(vpcsum_ctx* c) {
    Service& v = c->svc;
    if (v.mb.p) __atomic_store_n(&v.mb.p->cmd, kSvcStop, __ATOMIC_RELEASE);
    if (v.stream) {
        (void)hipStreamSynchronize(v.stream);   // the grid sees kSvcStop within a poll interval
        (void)hipStreamDestroy(v.stream);
    }
    if (v.ctr) (void)hipFree(v.ctr);
    c->svc = Service();   // the mailbox and the four buffers free themselves, in that order
}

int vpcsum_ctx_set_service(vpcsum_ctx_t* c, uint32_t idle_us) {
    try {
        if (!c) return fail("vpcsum_ctx_set_service: NULL context");
        std::lock_guard<std::mutex> lk(c->mu);
        VPC_ON_DEVICE(c->device);
        for (auto& s : c->slots)
            if (s.busy && slot_finish(c, s) != 0) return -1;
        svc_free(c);
        if (idle_us == 0) return 0;
        Service& v = c->svc;
        hipError_t e = hipSuccess;
        if ((e = v.mb.pin(sizeof(SvcMailbox))) != hipSuccess || (e = v.mb.map()) != hipSuccess ||
            (e = v.h_desc.pin((size_t)c->max_pkts * sizeof(vpcsum_desc_t))) != hipSuccess ||
            (e = v.h_out.pin((size_t)c->max_pkts * 4)) != hipSuccess ||
            (e = v.h_status.pin((size_t)c->max_pkts)) != hipSuccess ||
            (e = v.h_pre.pin(kSvcAuxBytes)) != hipSuccess ||
            (e = v.h_pre.map()) != hipSuccess || (e = v.h_desc.map()) != hipSuccess ||
            (e = v.h_out.map()) != hipSuccess || (e = v.h_status.map()) != hipSuccess ||
            (e = hipMalloc((void**)&v.ctr, 16)) != hipSuccess ||   // counter + command relay
            (e = hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking)) != hipSuccess) {
            svc_free(c);
            return hipfail(e, "vpcsum_ctx_set_service allocation");
        }
        memset((void*)v.mb.p, 0, sizeof(SvcMailbox));
        v.mb.p->desc = (uint64_t)(uintptr_t)v.h_desc.dev;
        v.mb.p->out = (uint64_t)(uintptr_t)v.h_out.dev;
        v.mb.p->status = (uint64_t)(uintptr_t)v.h_status.dev;
        v.mb.p->pre = (uint64_t)(uintptr_t)v.h_pre.dev;
        v.idle_ticks = (uint64_t)idle_us * 100u;   // s_memrealtime runs at 100 MHz
        const char* gs = getenv("VPCSUM_SVC_GRID");   // A/B tooling: the grid's workgroups (1..256)
        if (gs && atoi(gs) >= 1 && atoi(gs) <= 256) v.grid = (uint32_t)atoi(gs);
        const char* pm = getenv("VPCSUM_SVC_POLL");   // 0: round 5's acquire loads
        if (pm) v.poll = (uint32_t)atoi(pm) & 7u;
        const char* inl = getenv("VPCSUM_SVC_INLINE");
        v.inline_desc = !(inl && inl[0] == '0');
        const char* clamp = getenv("VPCSUM_SVC_CLAMP");   // A/B tooling: 1 = clamped frame loads
        const char* reld = getenv("VPCSUM_SVC_RELEASE_DONE");   // A/B tooling: 1 = release on count / done
        v.mb.p->opts = ((clamp && clamp[0] == '1') ? kSvcOptClampLoads : 0) | ((reld && reld[0] == '1') ? kSvcOptReleaseDone : 0);
        v.on = true;
        return 0;
    } VPC_CATCH("vpcsum_ctx_set_service")
}

int vpcsum_ctx_stats(vpcsum_ctx_t* c, uint64_t* service_batches, uint64_t* service_launches) {
    try {
        if (!c) return fail("vpcsum_ctx_stats: NULL context");
        std::lock_guard<std::mutex> lk(c->mu);
        if (service_batches) *service_batches = c->svc_batches;
        if (service_launches) *service_launches = c->svc_launches;
        return 0;
    } VPC_CATCH("vpcsum_ctx_stats")
}

int vpcsum_ctx_create(int device, uint64_t max_arena_bytes, uint32_t max_pkts, vpcsum_ctx_t** out) {
    try {
        if (!out) return fail("vpcsum_ctx_create: out is NULL");
        if (max_arena_bytes == 0 || max_pkts == 0) return fail("vpcsum_ctx_create: zero capacity");
        VPC_ON_DEVICE(device);
        vpcsum_ctx* c = new vpcsum_ctx();
        c->device = device;
        c->max_arena = max_arena_bytes;
        c->max_pkts = max_pkts;
        for (auto& s : c->slots) {
            hipError_t e = hipSuccess;
            if ((e = s.d_arena.alloc(max_arena_bytes + 64)) != hipSuccess ||
                (e = s.d_desc.alloc((size_t)max_pkts * sizeof(vpcsum_desc_t))) != hipSuccess ||
                (e = s.d_out.alloc((size_t)max_pkts * 4)) != hipSuccess ||
                (e = s.d_status.alloc((size_t)max_pkts)) != hipSuccess ||
                (e = s.h_desc.pin((size_t)max_pkts * sizeof(vpcsum_desc_t))) != hipSuccess ||
                (e = s.h_out.pin((size_t)max_pkts * 4)) != hipSuccess ||
                (e = s.h_status.pin((size_t)max_pkts)) != hipSuccess ||
                (e = s.h_desc.map()) != hipSuccess || (e = s.h_out.map()) != hipSuccess ||
                (e = s.h_status.map()) != hipSuccess ||
                (e = hipHostMalloc((void**)&s.h_arena.p, max_arena_bytes + 64, 0)) != hipSuccess ||
                (e = s.h_foff.pin((size_t)max_pkts * 8)) != hipSuccess ||
                (e = s.h_flen.pin((size_t)max_pkts * 4)) != hipSuccess ||
                (e = s.h_foff.map()) != hipSuccess || (e = s.h_flen.map()) != hipSuccess ||
                (e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess ||
                (e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) {
                for (auto& t : c->slots) slot_free(t);
                delete c;
                return hipfail(e, "vpcsum_ctx_create allocation");
            }
        }
        *out = c;
        return 0;
    } VPC_CATCH("vpcsum_ctx_create")
}

int vpcsum_ctx_destroy(vpcsum_ctx_t* c) {
    try {
        if (!c) return 0;
        DeviceScope on_dev(c->device);
        int rc = 0;
        {
            std::lock_guard<std::mutex> lk(c->mu);
            // batches still in flight complete first, as a wait would: their out / status (and a
            // staged batch's frames) reach the caller's buffers before anything is freed.  A failure
            // is reported, and the context is destroyed all the same.
            for (auto& s : c->slots)
                if (s.busy && slot_finish(c, s) != 0) rc = -1;
            svc_free(c);
            for (auto& s : c->slots) {
                if (s.stream) (void)hipStreamSynchronize(s.stream);
                slot_free(s);
            }
            // every page-lock reference this context holds goes, each failure reported (the caller
            // may free the arena once this returns: a range HIP still held as registered would be taken
            // for pinned memory by a later copy from whatever is allocated there)
            for (auto& r : c->registered)
                if (r.key && hostlock_release(r.key, "vpcsum_ctx_destroy") != 0) rc = -1;
        }
        delete c;
        return rc;
    } VPC_CATCH("vpcsum_ctx_destroy")
}

int vpcsum_ctx_register_arena(vpcsum_ctx_t* c, void* h_arena, uint64_t len) {
    try {
        if (!c || !h_arena || len == 0) return fail("vpcsum_ctx_register_arena: bad argument");
        std::lock_guard<std::mutex> lk(c->mu);
        VPC_ON_DEVICE(c->device);
        for (auto& r : c->registered)
            if (r.host == (uint8_t*)h_arena) return fail("vpcsum_ctx_register_arena: %p is registered already", h_arena);
        c->registered.reserve(c->registered.size() + 1);   // may throw: before anything is pinned
        uint8_t* key = nullptr;
        if (hostlock_acquire((uint8_t*)h_arena, len, &key, "vpcsum_ctx_register_arena") != 0) return -1;
        void* dev = nullptr;
        hipError_t e = hipHostGetDevicePointer(&dev, h_arena, 0);
        if (e != hipSuccess) {
            (void)hostlock_release(key, "vpcsum_ctx_register_arena");
            return hipfail(e, "hipHostGetDevicePointer");
        }
        c->registered.push_back({(uint8_t*)h_arena, len, (uint8_t*)dev, key});
        return 0;
    } VPC_CATCH("vpcsum_ctx_register_arena")
}

// A zero-copy batch (launched or on the service grid) may still read and write frames of a
// registered arena in place: finish every such batch of the context before a mapping goes away,
// and make the service re-read its parameters (they may name that arena) with its next batch.
// Caller holds c->mu on c's device.
static int ctx_quiesce_zero_copy(vpcsum_ctx* c) {
    for (auto& s : c->slots)
        if (s.busy && s.batch.zero_copy && slot_finish(c, s) != 0) return -1;
    c->svc.par_valid = false;
    return 0;
}

int vpcsum_ctx_unregister_arena(vpcsum_ctx_t* c, void* h_arena) {
    try {
        if (!c || !h_arena) return fail("vpcsum_ctx_unregister_arena: bad argument");
        std::lock_guard<std::mutex> lk(c->mu);
        VPC_ON_DEVICE(c->device);
        for (size_t i = 0; i < c->registered.size(); ++i) {
            if (c->registered[i].host == (uint8_t*)h_arena) {
                if (ctx_quiesce_zero_copy(c) != 0) return -1;
                uint8_t* key = c->registered[i].key;
                c->registered.erase(c->registered.begin() + i);
                return key ? hostlock_release(key, "vpcsum_ctx_unregister_arena") : 0;
            }
        }
        return fail("vpcsum_ctx_unregister_arena: arena not registered");
    } VPC_CATCH("vpcsum_ctx_unregister_arena")
}

// Device-side address of host range [p, p+len) if it lies in an arena registered with this context.
static uint8_t* mapped_dev(vpcsum_ctx* c, const uint8_t* p, uint64_t len) {
    for (auto& r : c->registered)
        if (p >= r.host && p + len <= r.host + r.len) return r.dev + (p - r.host);
    return nullptr;
}

// Whether the library may DMA straight from or to [p, p+len) (vpcsum_ctx_pipeline): only when this
// context registered it (its own registration or its group's), so the page-lock outlives the copy --
// vpcsum_ctx_unregister and destroy finish the context's batches before they unpin.  Memory
// page-locked by anyone else is never a DMA end: its owner may unpin or free it while the copy is
// in flight, which the library cannot see, so a staged submit copies it through the pinned staging
// (round 5 trusted hipPointerGetAttributes here; DESIGN_HISTORY.md "Round 6: the intermittent fault").
static bool is_registered(vpcsum_ctx* c, const uint8_t* p, uint64_t len) { return mapped_dev(c, p, len) != nullptr; }

static uint32_t svc_done(const Service& v) { return __atomic_load_n(&v.mb.p->done, __ATOMIC_ACQUIRE); }

// (Re)start the service grid: it treats batches after `seen` as new.  Only called while no grid
// of this context runs (stream idle), so the finished-wave counter can be cleared first.
static int svc_launch(vpcsum_ctx* c, uint32_t seen) {
    Service& v = c->svc;
    VPC_CHECK(hipMemsetAsync(v.ctr, 0, 16, v.stream), "service counter / relay reset");
    VPC_CHECK(launch_service(v.mb.dev, v.ctr, seen, v.idle_ticks, v.stream, v.grid, v.poll), "service launch");
    ++c->svc_launches;
    return 0;
}

// Wait until the service has completed batch `seq`.  A grid that left on its idle timeout while
// the batch was being posted may have done part of it: once the stream is idle the batch is run
// again from the start by a fresh grid (the sums do not read the fields they write).
#ifdef VPCSUM_SVC_STAMPS
// tooling build: per-batch durations of the service's steps (ns), medians per batch size at exit
static std::map<uint32_t, std::vector<uint64_t>> g_stamp_d[7];
static void stamps_print() {
    static const char* name[7] = {"host_post_to_done_seen_ns", "wg0_params_ns", "wg0_k1_ns", "wg0_release_ns",
                                  "wg0_atomic_ns", "wg0_seen_to_done_store_ns", "last_wg_seen_after_wg0_ns"};
    for (auto& kv : g_stamp_d[0]) {
        fprintf(stderr, "{\"n\": %u", kv.first);
        for (int i = 0; i < 7; ++i) {
            auto v = g_stamp_d[i][kv.first];
            std::sort(v.begin(), v.end());
            fprintf(stderr, ", \"%s\": %llu", name[i], (unsigned long long)v[v.size() / 2]);
        }
        fprintf(stderr, "}\n");
    }
}
#endif

static int svc_wait(vpcsum_ctx* c, uint32_t seq) {
    Service& v = c->svc;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 1; (int32_t)(svc_done(v) - seq) < 0; ++spin) {
        __builtin_ia32_pause();
        if ((spin & 255) != 0) continue;
        if (hipStreamQuery(v.stream) == hipSuccess && (int32_t)(svc_done(v) - seq) < 0) {
            if (svc_launch(c, seq - 1) != 0) return -1;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
            return fail("vpcsum service: batch %u not completed within 10 s", seq);
    }
#ifdef VPCSUM_SVC_STAMPS
    {
        static bool reg = false;
        if (!reg) { reg = true; atexit(stamps_print); }
        const uint64_t* s = (const uint64_t*)v.mb.p->stamp;
        const uint64_t s0 = s[0];
        const uint32_t n = v.t_n;
        g_stamp_d[0][n].push_back((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
            std::chrono::steady_clock::now() - v.t_post).count());
        for (int i = 1; i <= 4; ++i) g_stamp_d[i][n].push_back((s[i] - s[i - 1]) * 10);
        g_stamp_d[5][n].push_back((s[5] - s0) * 10);
        g_stamp_d[6][n].push_back((s[6] - s0) * 10);
    }
#endif
    return 0;
}

// Complete the slot's batch: wait for it, hand its results to the caller's buffers, and forget it.
static int slot_finish(vpcsum_ctx* c, Slot& s) {
    if (!s.busy) return 0;
    const Batch& b = s.batch;
    if (b.svc_seq) {
        if (svc_wait(c, b.svc_seq) != 0) return -1;
    } else {
        VPC_CHECK(hipEventSynchronize(s.done), "hipEventSynchronize");
    }
    for (uint32_t k = 0; k < b.n_back; ++k) memcpy(b.back[k].dst, b.back[k].src, b.back[k].bytes);
    // a staged batch's results go back into the caller's frames (a zero-copy batch wrote them in
    // place), by the status bytes of the staging
    if (b.scatter == Scatter::NatHeaders)
        return_nat_headers(b.user_arena, b.user_desc, s.h_arena.p, s.h_desc.p, s.h_status.p, b.n,
                           (b.mode & VPCSUM_NAT_TCP_REWRITES) != 0);
    else if (b.scatter == Scatter::CsumFields)
        place_checksums(b.user_arena, b.user_desc, s.h_out.p, s.h_status.p, b.n);
    s.batch = Batch();
    s.busy = false;
    return 0;
}

// The next ticket and its slot, whatever batch the slot still holds finished first.  nullptr: that
// batch failed (the message is set).
static Slot* slot_acquire(vpcsum_ctx* c, uint64_t* t) {
    *t = c->next_ticket++;
    Slot& s = c->slots[*t & 1];
    if (s.busy && slot_finish(c, s) != 0) return nullptr;
    return &s;
}

// Slot s now owns batch b, every field of it (what b does not name is reset, so nothing of the
// slot's previous batch survives).  A launched batch -- one not handed to the service -- is
// complete when `done`, recorded here behind its last launch or copy, has passed.
static int slot_commit(Slot& s, const Batch& b, uint64_t* ticket) {
    if (!b.svc_seq) VPC_CHECK(hipEventRecord(s.done, s.stream), "hipEventRecord");
    s.batch = b;
    s.busy = true;
    *ticket = b.ticket;
    return 0;
}

}  // extern "C"

// Buffers of the slot's per-packet scratch (Mapped or DeviceOnly), each allocated for max_pkts
// elements with the context's first batch that needs it, in the order given.
template <class Buf, class... More>
static int slot_scratch(vpcsum_ctx* c, const char* entry, Buf& buf, More&... more) {
    if (!buf.p) {
        const hipError_t e = buf.alloc((size_t)c->max_pkts * sizeof(*buf.p));
        if (e != hipSuccess) return fail("%s allocation: %s (%d)", entry, hipGetErrorString(e), (int)e);
    }
    if constexpr (sizeof...(More) > 0) return slot_scratch(c, entry, more...);
    return 0;
}

// The staged transfers of a batch on its slot's stream.  Up: the n descriptors of h_desc, the
// per-packet entries of h_rw (entry_bytes of them, 0: none) and the frames staged in h_arena.
// Down: the out words, if wanted, and the status bytes into the pinned staging.
static int stage_frames_up(Slot& s, uint64_t bytes) {
    if (bytes) VPC_CHECK(hipMemcpyAsync(s.d_arena.p, s.h_arena.p, bytes, hipMemcpyHostToDevice, s.stream), "H2D frames");
    return 0;
}

static int stage_up(Slot& s, uint32_t n, size_t entry_bytes, uint64_t frame_bytes) {
    VPC_CHECK(hipMemcpyAsync(s.d_desc.p, s.h_desc.p, (size_t)n * sizeof(vpcsum_desc_t), hipMemcpyHostToDevice, s.stream),
              "H2D descriptors");
    if (entry_bytes) VPC_CHECK(hipMemcpyAsync(s.d_rw.p, s.h_rw.p, entry_bytes, hipMemcpyHostToDevice, s.stream), "H2D entries");
    return stage_frames_up(s, frame_bytes);
}

static int stage_down(Slot& s, uint32_t n, bool out) {
    if (out) VPC_CHECK(hipMemcpyAsync(s.h_out.p, s.d_out.p, (size_t)n * 4, hipMemcpyDeviceToHost, s.stream), "D2H out");
    VPC_CHECK(hipMemcpyAsync(s.h_status.p, s.d_status.p, n, hipMemcpyDeviceToHost, s.stream), "D2H status");
    return 0;
}

// Where a batch's status bytes and out words will lie: the service's buffers or the slot's staging.
static HandBack status_of(vpcsum_ctx* c, Slot& s, bool svc, uint8_t* h_status, uint32_t n) {
    return {h_status, svc ? c->svc.h_status.p : s.h_status.p, n};
}
static HandBack out_of(vpcsum_ctx* c, Slot& s, bool svc, uint32_t* h_out, uint32_t n) {
    return {h_out, svc ? c->svc.h_out.p : s.h_out.p, (size_t)n * 4};
}

// Zero-copy batches of up to kZeroCopyWaveTeams packets run one wave per packet (variant 12, 64
// lanes x 4 predicated loads): the batch is a few PCIe round trips deep instead of K2's per-unit
// iterations, and no chunk is read twice over PCIe.
static CsumTune zero_copy_tune(uint32_t n) {
    CsumTune t;
    t.variant = n <= kZeroCopyWaveTeams ? 12 : 0;
    return t;
}

// The service runs one batch at a time: the previous one done, its results handed over, before its
// buffers are refilled.  (An idle grid stays resident beside launched batches: the stop round 5 had
// here is gone, DESIGN_HISTORY.md "Round 5: experiments" and "The context batch path in one piece".)
static int svc_drain(vpcsum_ctx* c) {
    for (auto& o : c->slots)
        if (o.busy && o.batch.svc_seq && slot_finish(c, o) != 0) return -1;
    return 0;
}

// Hand a zero-copy batch to the low-latency service (c->svc.on, n <= kSvcBatchMax): one batch at
// a time; descriptors (and pre-images) into the service's buffers, the parameter block if it
// changed, then the command word.  `base` is the device address of h_arena[0].  Caller holds c->mu
// on c's device; slot s is free and takes batch b (its n and mode are the batch's).
// form: kSvcFrames -- h_desc is the service's own buffer, filled with SvcFrameRec records (raw
// frames) -- with kSvcParse (parsed only, vpcsum_ctx_parse_frames) or kSvcHsum.
static int svc_post(vpcsum_ctx* c, Slot& s, Batch b, const uint8_t* h_arena, uint64_t arena_len, uint8_t* base,
                    const vpcsum_desc_t* h_desc, const void* h_pre, uint32_t pre_fmt, uint64_t form, uint64_t* ticket) {
    Service& v = c->svc;
    SvcMailbox* mb = v.mb.p;
    const uint32_t n = b.n, mode = b.mode;
    if (!(form & kSvcFrames)) memcpy(v.h_desc.p, h_desc, (size_t)n * sizeof(vpcsum_desc_t));
    uint64_t cmd = form;
    if (h_pre) {
        // the pre-images, each F_PRE frame's stored L4 sum copied into its entry's spare bytes
        // (vpcsum_pre4_t rsv[1..2], vpcsum_pre_t rsv[0..1]): the kernel takes the sum from there,
        // so a batch re-run by a fresh grid (svc_wait) computes from the same input
        const size_t esz = pre_fmt == VPCSUM_PRE_FMT_PRE ? sizeof(vpcsum_pre_t) : sizeof(vpcsum_pre4_t);
        const size_t at = pre_fmt == VPCSUM_PRE_FMT_PRE ? offsetof(vpcsum_pre_t, rsv) : offsetof(vpcsum_pre4_t, rsv) + 1;
        memcpy(v.h_pre.p, h_pre, (size_t)n * esz);
        for (uint32_t i = 0; i < n; ++i) {
            const vpcsum_desc_t& d = h_desc[i];
            const int fld = l4_field_host(d.l4_proto);
            if (!(d.flags & VPCSUM_F_PRE) || fld < 0 || !desc_in_arena(d, arena_len) ||
                (uint32_t)d.l4_off + fld + 2u > d.l3_len)
                continue;   // no L4 sum to update, or refused by the kernel
            memcpy((uint8_t*)v.h_pre.p + (size_t)i * esz + at, h_arena + d.l3_off + d.l4_off + fld, 2);
        }
        cmd |= kSvcPre | (pre_fmt == VPCSUM_PRE_FMT_PRE ? kSvcPreFmt : 0);
    }
    const uint64_t par[3] = {(uint64_t)(uintptr_t)base, arena_len, (mode & VPCSUM_MODE_WRITE) ? (uint64_t)(uintptr_t)base : 0};
    if (!v.par_valid || memcmp(par, v.par, sizeof(par)) != 0) {
        mb->arena = par[0];
        mb->arena_len = par[1];
        mb->arena_w = par[2];
        memcpy(v.par, par, sizeof(par));
        v.par_valid = true;
        cmd |= kSvcParams;
    }
    const uint32_t seq = v.posted + 1 ? v.posted + 1 : 1;
    // the first descriptors ride in the command's line, tagged with the batch.  All of them are
    // rewritten for every batch, so a stale one always carries the previous batch's tag; the high
    // word (with the tag) is stored after the low one.
    for (int k = 0; k < kSvcInlineDesc; ++k) {
        vpcsum_desc_t d;
        if ((uint32_t)k < n) memcpy(&d, &h_desc[k], sizeof(d));
        else memset(&d, 0, sizeof(d));
        d.rsv = (uint8_t)seq;
        uint64_t w[2];
        memcpy(w, &d, sizeof(w));
        uint64_t* dst = reinterpret_cast<uint64_t*>(&mb->idesc[k]);
        __atomic_store_n(&dst[0], w[0], __ATOMIC_RELAXED);
        __atomic_store_n(&dst[1], w[1], __ATOMIC_RELEASE);
    }
    cmd |= seq | ((uint64_t)n << 32) | ((mode & VPCSUM_MODE_VERIFY) ? kSvcVerify : 0) |
           (v.inline_desc && n <= (uint32_t)kSvcInlineDesc ? kSvcInline : 0);
#ifdef VPCSUM_SVC_STAMPS
    v.t_post = std::chrono::steady_clock::now();
    v.t_n = n;
#endif
    __atomic_store_n(&mb->cmd, cmd, __ATOMIC_RELEASE);
    v.posted = seq;
    ++c->svc_batches;
    if (hipStreamQuery(v.stream) == hipSuccess && svc_launch(c, seq - 1) != 0) return -1;
    b.zero_copy = true;
    b.svc_seq = seq;
    return slot_commit(s, b, ticket);
}

// A small batch of raw frames (egress, RX verify or RX parse) to the service grid: one SvcFrameRec
// per frame in the service's descriptor buffer -- offset, length, and the frame's own flags
// (h_flags) or `flags` for all -- then svc_post.  The results stay in the service's buffers until
// slot_finish hands them over; the frames themselves are written in place through the mapping.
static int svc_post_frames(vpcsum_ctx* c, Slot& s, const Batch& b, uint64_t arena_len, uint8_t* base,
                           const uint64_t* h_off, const uint32_t* h_len, const uint8_t* h_flags, uint8_t flags,
                           uint64_t form, uint64_t* ticket) {
    if (svc_drain(c) != 0) return -1;
    SvcFrameRec* r = reinterpret_cast<SvcFrameRec*>(c->svc.h_desc.p);
    for (uint32_t i = 0; i < b.n; ++i) {
        SvcFrameRec x;
        memset(&x, 0, sizeof(x));
        x.off = h_off[i];
        x.len = h_len[i];
        x.flags = h_flags ? h_flags[i] : flags;
        memcpy(&r[i], &x, sizeof(x));
    }
    return svc_post(c, s, b, nullptr, arena_len, base, c->svc.h_desc.p, nullptr, 0, kSvcFrames | form, ticket);
}

// The shared start of the descriptor entries (submit, submit_pre, nat_submit), in two parts around
// the checks an entry has of its own.  desc_args: the arguments every one of them refuses, under the
// entry's name (`also`: the array it needs besides the descriptors; `nulls` names them all).
static int desc_args(const vpcsum_ctx* c, const char* what, const char* nulls, const void* h_arena, const void* h_desc,
                     const void* also, uint32_t n, const uint64_t* ticket) {
    if (!c || !ticket) return fail("%s: NULL context or ticket", what);
    if (n > c->max_pkts) return fail("%s: %u packets > capacity %u", what, n, c->max_pkts);
    if (n && (!h_arena || !h_desc || !also)) return fail("%s: NULL %s", what, nulls);
    return 0;
}

// desc_entry: the next slot, and where the batch's frames are.  body(s, b, sp, base) then runs the
// batch under c->mu on c's device; b carries the ticket, n, mode and the caller's frames and
// descriptors, sp is the span of the descriptors in the arena, and base the device address of
// h_arena[0] when that span lies in a registered arena (zero-copy), else NULL (staged).
template <class Body>
static int desc_entry(vpcsum_ctx* c, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, uint32_t n,
                      uint32_t mode, Body body) {
    std::lock_guard<std::mutex> lk(c->mu);
    VPC_ON_DEVICE(c->device);
    Batch b;
    Slot* s = slot_acquire(c, &b.ticket);
    if (!s) return -1;
    b.n = n;
    b.mode = mode;
    b.user_arena = h_arena;
    b.user_desc = h_desc;
    const BatchSpan sp = batch_span(h_desc, n, arena_len);
    uint8_t* dev_arena = sp.hi > sp.lo ? mapped_dev(c, h_arena + sp.lo, sp.hi - sp.lo) : nullptr;
    return body(*s, b, sp, dev_arena ? dev_arena - sp.lo : nullptr);
}

// The frames of a staged descriptor batch (batch_plan.h), into the slot's pinned staging: a sparse
// batch in a large pageable arena as its gathered 16-B blocks, any other as the span [lo, hi).
// s.h_desc holds the descriptors rebased to the staging (out of the span: UINT64_MAX, refused by the
// kernels); *dev_len is how many bytes stage_frames_up carries.
static int stage_desc_frames(vpcsum_ctx* c, Slot& s, const char* what, const uint8_t* h_arena, uint64_t arena_len,
                             const vpcsum_desc_t* h_desc, uint32_t n, const BatchSpan& sp, uint64_t* dev_len) {
    const uint64_t lo = sp.lo, span = sp.hi - sp.lo;
    if (span > 2 * sp.used + (64u << 10)) {
        // sparse batch in a large pageable arena: gather the touched 16-B blocks only
        const int64_t staged = gather_blocks(h_arena, arena_len, h_desc, n, s.h_desc.p, s.h_arena.p, c->max_arena);
        if (staged < 0) return fail("%s: gathered batch exceeds capacity", what);
        *dev_len = (uint64_t)staged;
        return 0;
    }
    if (span > c->max_arena)
        return fail("%s: batch spans %llu bytes > capacity %llu", what, (unsigned long long)span, (unsigned long long)c->max_arena);
    // descriptors rebased to the device copy of [lo, hi)
    for (uint32_t i = 0; i < n; ++i) {
        s.h_desc.p[i] = h_desc[i];
        if (h_desc[i].l3_off >= lo) s.h_desc.p[i].l3_off = h_desc[i].l3_off - lo;
        else s.h_desc.p[i].l3_off = UINT64_MAX;   // out of span -> BAD in the kernel
    }
    // through the pinned staging, always: the span lies in no arena this context registered, and the
    // library never DMAs from memory it did not register (is_registered)
    if (span) memcpy(s.h_arena.p, h_arena + lo, span);
    *dev_len = span;
    return 0;
}

extern "C" {

int vpcsum_ctx_submit(vpcsum_ctx_t* c, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, uint32_t n,
                      uint32_t* h_out, uint8_t* h_status, uint32_t mode, uint64_t* ticket) {
    try {
        if (desc_args(c, "vpcsum_ctx_submit", "arena or descriptors", h_arena, h_desc, h_desc, n, ticket) != 0) return -1;
        if (mode & ~(VPCSUM_MODE_VERIFY | VPCSUM_MODE_WRITE)) return fail("vpcsum_ctx_submit: bad mode 0x%x", mode);
        return desc_entry(c, h_arena, arena_len, h_desc, n, mode, [&](Slot& s, Batch& b, const BatchSpan& sp, uint8_t* base) {
            const bool svc = base && c->svc.on && n <= kSvcBatchMax;
            b.hand_back({status_of(c, s, svc, h_status, n), out_of(c, s, svc, h_out, n)});
            if (base) {
                // Zero-copy: the frames live in a page-locked, mapped arena (an AF_XDP umem).  The
                // kernel reads them over PCIe in place, takes the descriptors from and writes the
                // results to pinned staging, and with MODE_WRITE stores the checksum fields straight
                // into the frames -- no DMA copy in either direction.
                if (svc)
                    return svc_drain(c) != 0 ? -1 : svc_post(c, s, b, h_arena, arena_len, base, h_desc, nullptr, 0, 0, ticket);
                memcpy(s.h_desc.p, h_desc, (size_t)n * sizeof(vpcsum_desc_t));
                // no out words asked for (an ingress verify: the status bytes are the result): none written
                VPC_CHECK(launch_csum(base, arena_len, s.h_desc.dev, n, h_out ? s.h_out.dev : nullptr, s.h_status.dev, nullptr,
                                      (mode & VPCSUM_MODE_VERIFY) != 0, (mode & VPCSUM_MODE_WRITE) ? base : nullptr,
                                      zero_copy_tune(n), s.stream),
                          "checksum launch (zero-copy)");
                b.zero_copy = true;
            } else {
                uint64_t dev_len = 0;
                if (stage_desc_frames(c, s, "vpcsum_ctx_submit", h_arena, arena_len, h_desc, n, sp, &dev_len) != 0) return -1;
                if (stage_up(s, n, 0, dev_len) != 0) return -1;
                // the out words travel when the caller asked for them or MODE_WRITE places them in the frames
                const bool want_out = h_out || (mode & VPCSUM_MODE_WRITE);
                VPC_CHECK(launch_csum(s.d_arena.p, dev_len, s.d_desc.p, n, want_out ? s.d_out.p : nullptr, s.d_status.p, nullptr,
                                      (mode & VPCSUM_MODE_VERIFY) != 0, nullptr, CsumTune{}, s.stream),
                          "checksum launch");
                if (stage_down(s, n, want_out) != 0) return -1;
                if (mode & VPCSUM_MODE_WRITE) b.scatter = Scatter::CsumFields;
            }
            return slot_commit(s, b, ticket);
        });
    } VPC_CATCH("vpcsum_ctx_submit")
}

int vpcsum_ctx_submit_pre(vpcsum_ctx_t* c, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                          const void* h_pre, uint32_t pre_fmt, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                          uint32_t mode, uint64_t* ticket) {
    try {
        if (desc_args(c, "vpcsum_ctx_submit_pre", "arena, descriptors or pre-images", h_arena, h_desc, h_pre, n, ticket) != 0)
            return -1;
        if (pre_fmt > VPCSUM_PRE_FMT_PRE) return fail("vpcsum_ctx_submit_pre: bad pre_fmt %u", pre_fmt);
        if (mode & ~VPCSUM_MODE_WRITE) return fail("vpcsum_ctx_submit_pre: bad mode 0x%x (COMPUTE or WRITE)", mode);
        uint32_t npre = 0;
        for (uint32_t i = 0; i < n; ++i) npre += (h_desc[i].flags & VPCSUM_F_PRE) ? 1u : 0u;
        // no pre-image in the batch: a plain submit (the service grid may take it)
        if (npre == 0) return vpcsum_ctx_submit(c, h_arena, arena_len, h_desc, n, h_out, h_status, mode, ticket);
        const size_t esz = pre_fmt == VPCSUM_PRE_FMT_PRE ? sizeof(vpcsum_pre_t) : sizeof(vpcsum_pre4_t);
        const bool full = npre < n;   // descriptors the checksum kernel sums in full
        return desc_entry(c, h_arena, arena_len, h_desc, n, mode, [&](Slot& s, Batch& b, const BatchSpan&, uint8_t* base) {
            const uint32_t wr = mode & VPCSUM_MODE_WRITE;
            const bool svc = base && c->svc.on && n <= kSvcBatchMax;
            b.hand_back({status_of(c, s, svc, h_status, n), out_of(c, s, svc, h_out, n)});
            // a small flush from the registered umem: the service grid, F_PRE frames and the others in
            // one batch (kernels.hip svc_pre_packet)
            if (svc)
                return svc_drain(c) != 0 ? -1 : svc_post(c, s, b, h_arena, arena_len, base, h_desc, h_pre, pre_fmt, 0, ticket);
            if (slot_scratch(c, "vpcsum_ctx_submit_pre", s.h_rw, s.d_rw) != 0) return -1;
            memcpy(s.h_rw.p, h_pre, (size_t)n * esz);
            if (base) {
                // registered arena (umem): in place; an F_PRE packet's header is all that crosses PCIe
                memcpy(s.h_desc.p, h_desc, (size_t)n * sizeof(vpcsum_desc_t));
                if (full)
                    VPC_CHECK(launch_csum(base, arena_len, s.h_desc.dev, n, s.h_out.dev, s.h_status.dev, nullptr, false,
                                          wr ? base : nullptr, zero_copy_tune(n), s.stream),
                              "checksum launch (zero-copy)");
                VPC_CHECK(launch_pre(base, arena_len, s.h_desc.dev, s.h_rw.dev, n, s.h_out.dev, s.h_status.dev,
                                     pre_build(wr, (int)pre_fmt), s.stream),
                          "pre-image launch (zero-copy)");
                b.zero_copy = true;
            } else {
                // staged: each packet's 16-B blocks gathered into the pinned staging -- of an F_PRE
                // packet only its header (pre_staged_len; its descriptor's l3_len cut to that)
                const int64_t pos = gather_blocks(
                    h_arena, arena_len, h_desc, n, s.h_desc.p, s.h_arena.p, c->max_arena, [&](uint32_t i, const vpcsum_desc_t& d) {
                        const uint8_t* e = (const uint8_t*)h_pre + (size_t)i * esz;
                        bool cut;
                        const uint32_t take = pre_staged_len(h_arena, d, e, pre_fmt, &cut);
                        if (cut && (pre_entry_mask(e, pre_fmt) & VPCSUM_PRE_HSUM)) {
                            // the kernel checks the record's segment length against the descriptor's,
                            // which is cut here: check it against the real one on the host, and hand the
                            // kernel the cut length (or, on a mismatch, a record it refuses)
                            vpcsum_hsum_t hs;
                            uint8_t* se = (uint8_t*)s.h_rw.p + (size_t)i * esz;
                            memcpy(&hs, se, sizeof(hs));
                            if (hs.l4_len == (uint32_t)d.l3_len - d.l4_off) hs.l4_len = (uint16_t)(take - d.l4_off);
                            else hs.l2_len = 0;
                            memcpy(se, &hs, sizeof(hs));
                        }
                        return take;
                    });
                if (pos < 0) return fail("vpcsum_ctx_submit_pre: gathered batch exceeds capacity");
                if (stage_up(s, n, (size_t)n * esz, (uint64_t)pos) != 0) return -1;
                if (full)
                    VPC_CHECK(launch_csum(s.d_arena.p, pos, s.d_desc.p, n, s.d_out.p, s.d_status.p, nullptr, false, nullptr,
                                          CsumTune{}, s.stream),
                              "checksum launch");
                // the sums go back through out: slot_finish writes them into the caller's frames
                VPC_CHECK(launch_pre(s.d_arena.p, pos, s.d_desc.p, s.d_rw.p, n, s.d_out.p, s.d_status.p, pre_build(0, (int)pre_fmt),
                                     s.stream),
                          "pre-image launch");
                if (stage_down(s, n, true) != 0) return -1;
                if (wr) b.scatter = Scatter::CsumFields;
            }
            return slot_commit(s, b, ticket);
        });
    } VPC_CATCH("vpcsum_ctx_submit_pre")
}

int vpcsum_ctx_wait(vpcsum_ctx_t* c, uint64_t ticket) {
    try {
        if (!c) return fail("vpcsum_ctx_wait: NULL context");
        std::lock_guard<std::mutex> lk(c->mu);
        VPC_ON_DEVICE(c->device);
        Slot& s = c->slots[ticket & 1];
        if (!s.busy || s.batch.ticket != ticket) {
            if (ticket == 0 || ticket >= c->next_ticket) return fail("vpcsum_ctx_wait: unknown ticket %llu", (unsigned long long)ticket);
            return 0;   // already completed
        }
        return slot_finish(c, s);
    } VPC_CATCH("vpcsum_ctx_wait")
}

}  // extern "C"

// The shared start of the frame-table entries (verify, egress, parse): the arguments checked under
// the entry's name (`also`: the array the entry needs besides the table; `nulls` names them all),
// the registered arena's mapping, the next slot, and -- for a batch that is launched, not handed to
// the service grid (`svc`) -- the frame table staged.  body(s, b, base, svc) then runs the batch
// under c->mu on c's device; b carries the ticket and n, and is zero-copy.
template <class Body>
static int frames_entry(vpcsum_ctx* c, const char* what, const char* nulls, const uint8_t* h_arena, uint64_t arena_len,
                        const uint64_t* h_frame_off, const uint32_t* h_frame_len, const void* also, uint32_t n,
                        uint64_t* ticket, Body body, bool may_svc = true) {
    if (!c || !ticket) return fail("%s: NULL context or ticket", what);
    if (n > c->max_pkts) return fail("%s: %u frames > capacity %u", what, n, c->max_pkts);
    if (n && (!h_arena || !h_frame_off || !h_frame_len || !also)) return fail("%s: NULL %s", what, nulls);
    std::lock_guard<std::mutex> lk(c->mu);
    VPC_ON_DEVICE(c->device);
    uint8_t* base = n ? mapped_dev(c, h_arena, arena_len) : nullptr;
    if (n && !base) return fail("%s: the arena must be registered (vpcsum_ctx_register_arena)", what);
    Batch b;
    Slot* s = slot_acquire(c, &b.ticket);
    if (!s) return -1;
    b.n = n;
    b.zero_copy = true;   // read, and written, in place through the mapping
    const bool svc = may_svc && n && c->svc.on && n <= kSvcBatchMax;
    if (n && !svc) {
        memcpy(s->h_foff.p, h_frame_off, (size_t)n * 8);
        memcpy(s->h_flen.p, h_frame_len, (size_t)n * 4);
    }
    return body(*s, b, base, svc);
}

extern "C" {

// vpcsum_ctx_verify_frames / _hsum: h_hsum NULL = no header sums
static int ctx_verify_frames(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const uint64_t* h_frame_off,
                             const uint32_t* h_frame_len, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                             vpcsum_hsum_t* h_hsum, uint64_t* ticket, const char* what) {
    return frames_entry(c, what, "arena, frame table or status", h_arena, arena_len, h_frame_off, h_frame_len, h_status, n,
                        ticket, [&](Slot& s, Batch b, uint8_t* base, bool svc) {
        if (h_hsum && n && slot_scratch(c, what, s.h_hs) != 0) return -1;
        b.mode = VPCSUM_MODE_VERIFY;
        // the header sums: the service's aux buffer, or the slot's staging
        b.hand_back({status_of(c, s, svc, h_status, n), out_of(c, s, svc, h_out, n),
                     {h_hsum, svc ? (const void*)c->svc.h_pre.p : (const void*)s.h_hs.p, (size_t)n * sizeof(vpcsum_hsum_t)}});
        // a small received batch: the service grid parses and verifies each frame
        // (kernels.hip svc_frame_packet), the sums into its own buffer (copied out only with h_out),
        // the header sums into its aux buffer
        if (svc)
            return svc_post_frames(c, s, b, arena_len, base, h_frame_off, h_frame_len, nullptr, VPCSUM_F_IP | VPCSUM_F_L4,
                                   h_hsum ? kSvcHsum : 0, ticket);
        if (n) {
            // parse the frames where they lie (zero-copy), then verify the descriptors it built
            VPC_CHECK(launch_parse_ether(base, arena_len, s.h_foff.dev, s.h_flen.dev, n, VPCSUM_F_IP | VPCSUM_F_L4, s.d_desc.p,
                                         nullptr, nullptr, s.stream, nullptr, h_hsum ? s.h_hs.dev : nullptr),
                      "parse launch");
            // h_out NULL: the status bytes alone (the out words are 4 of the 5 result bytes a packet writes)
            VPC_CHECK(launch_csum(base, arena_len, s.d_desc.p, n, h_out ? s.h_out.dev : nullptr, s.h_status.dev, nullptr,
                                  true, nullptr, zero_copy_tune(n), s.stream),
                      "verify launch");
        }
        return slot_commit(s, b, ticket);
    });
}

int vpcsum_ctx_verify_frames(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const uint64_t* h_frame_off,
                             const uint32_t* h_frame_len, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                             uint64_t* ticket) {
    try {
        return ctx_verify_frames(c, h_arena, arena_len, h_frame_off, h_frame_len, n, h_out, h_status, nullptr, ticket,
                                 "vpcsum_ctx_verify_frames");
    } VPC_CATCH("vpcsum_ctx_verify_frames")
}

int vpcsum_ctx_verify_frames_hsum(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const uint64_t* h_frame_off,
                                  const uint32_t* h_frame_len, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                                  vpcsum_hsum_t* h_hsum, uint64_t* ticket) {
    try {
        if (n && !h_hsum) return fail("vpcsum_ctx_verify_frames_hsum: NULL header-sum array");
        return ctx_verify_frames(c, h_arena, arena_len, h_frame_off, h_frame_len, n, h_out, h_status, h_hsum, ticket,
                                 "vpcsum_ctx_verify_frames_hsum");
    } VPC_CATCH("vpcsum_ctx_verify_frames_hsum")
}

int vpcsum_ctx_egress_frames(vpcsum_ctx_t* c, uint8_t* h_arena, uint64_t arena_len, const uint64_t* h_frame_off,
                             const uint32_t* h_frame_len, const uint8_t* h_frame_flags, uint32_t n, uint32_t* h_out,
                             uint8_t* h_status, uint64_t* ticket) {
    try {
        return frames_entry(c, "vpcsum_ctx_egress_frames", "arena, frame table or flags", h_arena, arena_len, h_frame_off,
                            h_frame_len, h_frame_flags, n, ticket, [&](Slot& s, Batch b, uint8_t* base, bool svc) {
            b.mode = VPCSUM_MODE_WRITE;
            b.hand_back({status_of(c, s, svc, h_status, n), out_of(c, s, svc, h_out, n)});
            // a small flush: the service grid parses and sums each frame (kernels.hip svc_frame_packet)
            if (svc)
                return svc_post_frames(c, s, b, arena_len, base, h_frame_off, h_frame_len, h_frame_flags, 0, 0, ticket);
            if (n) {
                // the frames' own flags ride in the status staging: the parse reads them before the
                // checksum kernel, later on the same stream, overwrites them with the statuses
                memcpy(s.h_status.p, h_frame_flags, n);
                VPC_CHECK(launch_parse_ether(base, arena_len, s.h_foff.dev, s.h_flen.dev, n, 0, s.d_desc.p, nullptr, nullptr,
                                             s.stream, s.h_status.dev),
                          "parse launch");
                VPC_CHECK(launch_csum(base, arena_len, s.d_desc.p, n, s.h_out.dev, s.h_status.dev, nullptr, false,
                                      base, zero_copy_tune(n), s.stream),
                          "checksum launch");
            }
            return slot_commit(s, b, ticket);
        });
    } VPC_CATCH("vpcsum_ctx_egress_frames")
}

int vpcsum_ctx_parse_frames(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const uint64_t* h_frame_off,
                            const uint32_t* h_frame_len, uint32_t n, vpcsum_desc_t* h_desc, uint8_t* h_status,
                            vpcsum_tuple_t* h_tuples, uint64_t* ticket) {
    try {
        return frames_entry(c, "vpcsum_ctx_parse_frames", "arena or frame table", h_arena, arena_len, h_frame_off,
                            h_frame_len, h_arena, n, ticket, [&](Slot& s, Batch b, uint8_t* base, bool svc) {
            if (slot_scratch(c, "vpcsum_ctx_parse_frames", s.h_tu) != 0) return -1;
            // descriptors and tuples: the pinned staging, or the service's aux buffer (the tuples
            // behind room for kSvcBatchMax descriptors)
            const uint8_t* aux = c->svc.h_pre.p;
            b.hand_back({status_of(c, s, svc, h_status, n),
                         {h_desc, svc ? (const void*)aux : (const void*)s.h_desc.p, (size_t)n * sizeof(vpcsum_desc_t)},
                         {h_tuples, svc ? (const void*)(aux + (size_t)kSvcBatchMax * sizeof(vpcsum_desc_t)) : (const void*)s.h_tu.p,
                          (size_t)n * sizeof(vpcsum_tuple_t)}});
            // a small received batch: the service grid parses each frame (kernels.hip svc_frame_packet)
            if (svc)
                return svc_post_frames(c, s, b, arena_len, base, h_frame_off, h_frame_len, nullptr, VPCSUM_F_IP | VPCSUM_F_L4,
                                       kSvcParse, ticket);
            if (n) {
                // parsed where the frames lie (zero-copy); results straight into the pinned staging
                VPC_CHECK(launch_parse_ether(base, arena_len, s.h_foff.dev, s.h_flen.dev, n, VPCSUM_F_IP | VPCSUM_F_L4,
                                             s.h_desc.dev, s.h_status.dev, s.h_tu.dev, s.stream),
                          "parse launch");
            }
            return slot_commit(s, b, ticket);
        });
    } VPC_CATCH("vpcsum_ctx_parse_frames")
}

int vpcsum_ctx_nat_submit(vpcsum_ctx_t* c, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                          const vpcsum_nat_t* h_rw, uint32_t n, uint8_t* h_status, uint32_t nat_mode, uint64_t* ticket) {
    try {
        if (desc_args(c, "vpcsum_ctx_nat_submit", "arena, descriptors or rewrites", h_arena, h_desc, h_rw, n, ticket) != 0)
            return -1;
        if (nat_mode & ~kNatCtxModeAccept)
            return fail("vpcsum_ctx_nat_submit: bad nat_mode 0x%x", nat_mode);
        // without the status bytes the caller would never see S_MSS_ABSENT, its part of the clamp
        if ((nat_mode & VPCSUM_NAT_TCP_REWRITES) && !h_status)
            return fail("vpcsum_ctx_nat_submit: VPCSUM_NAT_TCP_REWRITES needs a status buffer");
        return desc_entry(c, h_arena, arena_len, h_desc, n, nat_mode, [&](Slot& s, Batch& b, const BatchSpan&, uint8_t* base) {
            b.hand_back({status_of(c, s, false, h_status, n)});
            if (slot_scratch(c, "vpcsum_ctx_nat_submit", s.h_rw, s.d_rw) != 0) return -1;
            memcpy(s.h_rw.p, h_rw, (size_t)n * sizeof(vpcsum_nat_t));
            if (base) {
                // the frames live in a registered (page-locked, mapped) arena: rewritten where they lie
                memcpy(s.h_desc.p, h_desc, (size_t)n * sizeof(vpcsum_desc_t));
                if (n && nat_run(base, arena_len, s.h_desc.dev, s.h_rw.dev, 1, n, s.h_status.dev, nat_mode, s.stream) != 0)
                    return -1;
                b.zero_copy = true;
            } else {
                // staged: each packet's 16-B blocks gathered into the pinned staging, rewritten on the
                // device, and the whole gathered batch copied back (the headers return at wait: L3 header
                // through the L4 checksum field, the TCP header too under VPCSUM_NAT_TCP_REWRITES)
                const int64_t pos = gather_blocks(h_arena, arena_len, h_desc, n, s.h_desc.p, s.h_arena.p, c->max_arena);
                if (pos < 0) return fail("vpcsum_ctx_nat_submit: batch exceeds the staging capacity");
                if (n) {
                    if (stage_up(s, n, (size_t)n * sizeof(vpcsum_nat_t), (uint64_t)pos) != 0) return -1;
                    if (nat_run(s.d_arena.p, pos, s.d_desc.p, s.d_rw.p, 1, n, s.d_status.p, nat_mode, s.stream) != 0) return -1;
                    if (pos) VPC_CHECK(hipMemcpyAsync(s.h_arena.p, s.d_arena.p, pos, hipMemcpyDeviceToHost, s.stream), "D2H frames");
                    if (stage_down(s, n, false) != 0) return -1;
                }
                b.scatter = Scatter::NatHeaders;
            }
            return slot_commit(s, b, ticket);
        });
    } VPC_CATCH("vpcsum_ctx_nat_submit")
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// NAT flow table (vpcsum.h vpcsum_flowtab_*): the host logic is flow_table.h's FlowTable over a
// pinned mirror of the device table; an update changes the mirror, copies the slots it dirtied (in
// runs of neighbours) on the caller's stream and waits for them, so the mirror is never written
// while a copy reads it.  `touched` is one byte per flow id, set by the lookup kernel.
// ------------------------------------------------------------------------------------------
struct vpcsum_flowtab {
    int device = 0;
    uint32_t max_flows = 0;
    FlowSlot* h_slots = nullptr;    // pinned mirror
    FlowSlot* d_slots = nullptr;
    uint8_t* d_touched = nullptr;   // max_flows bytes
    uint8_t* h_touched = nullptr;   // pinned, collect's copy
    std::unique_ptr<FlowTable> t;
    bool resync = false;            // a copy of changed slots failed: the next update copies the whole table
    std::mutex mu;
};

static void flowtab_free(vpcsum_flowtab* f) {
    if (f->h_slots) (void)hipHostFree(f->h_slots);
    if (f->d_slots) (void)hipFree(f->d_slots);
    if (f->d_touched) (void)hipFree(f->d_touched);
    if (f->h_touched) (void)hipHostFree(f->h_touched);
    delete f;
}

// [a, b) runs of consecutive values in the sorted, duplicate-free v
template <class F>
static int for_runs(const std::vector<uint32_t>& v, F f) {
    for (size_t i = 0; i < v.size();) {
        size_t j = i + 1;
        while (j < v.size() && v[j] == v[j - 1] + 1) ++j;
        if (f(v[i], v[j - 1] + 1) != 0) return -1;
        i = j;
    }
    return 0;
}

static void sort_unique(std::vector<uint32_t>& v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

// The lookup of a batch under f->mu (max_probe and the launch are one step against a concurrent
// update); the caller is on the table's device.  d_fp != NULL: the lookup that also writes the
// flows' Fastpath records.
static int flow_lookup(vpcsum_flowtab* f, const vpcsum_tuple_t* d_tuples, uint32_t n, vpcsum_nat_t* d_rw, uint8_t* d_verdict,
                       vpcsum_fastpath_t* d_fp, hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    VPC_CHECK(launch_flow_lookup(f->d_slots, f->t->mask(), f->t->max_probe(), f->d_touched, d_tuples, n, d_rw, d_verdict,
                                 d_fp, s),
              "flow lookup launch");
    return 0;
}

// vpcsum_flow_lookup_async (fp false, d_fp NULL) / vpcsum_flow_lookup_fp_async
static int flow_lookup_async(const char* what, bool fp, vpcsum_flowtab* f, const vpcsum_tuple_t* d_tuples, uint32_t n,
                             vpcsum_nat_t* d_rw, uint8_t* d_verdict, vpcsum_fastpath_t* d_fp, void* stream) {
    if (!f) return fail("%s: NULL table", what);
    if (n == 0) return 0;
    if (!d_tuples || !d_rw || !d_verdict || (fp && !d_fp))
        return fail("%s: NULL tuples, entries%s", what, fp ? ", verdicts or Fastpath records" : " or verdicts");
    if (((uintptr_t)d_tuples | (uintptr_t)d_rw | (uintptr_t)d_fp) & 3)
        return fail("%s: tuples / entries%s not 4-byte aligned", what, fp ? " / Fastpath records" : "");
    if (n > (1u << 28)) return fail("%s: %u packets > 2^28", what, n);
    VPC_ON_DEVICE(f->device);
    return flow_lookup(f, d_tuples, n, d_rw, d_verdict, d_fp, (hipStream_t)stream);
}

// The mirror's changed slots to the device on stream s, and the wait for them (so that the mirror is
// not written again while a copy reads it); caller holds f->mu on f's device.  `freed`: the flow ids
// an update erased, whose marks go with them (an id may be handed to another flow).
static int flowtab_push(vpcsum_flowtab* f, FlowDirty& dirty, std::vector<uint32_t>& freed, hipStream_t s, const char* what) {
    sort_unique(dirty.idx);
    sort_unique(freed);
    // the whole table in one copy instead of its runs: a bulk load (an eighth of the slots or
    // more changed), more slots written than `dirty` had room for, or an earlier copy that failed
    const bool whole = dirty.all || f->resync || dirty.idx.size() >= f->t->slots() / 8u;
    f->resync = true;   // until the copies below are queued
    int rc = for_runs(freed, [&](uint32_t a, uint32_t b) {
        const hipError_t e = hipMemsetAsync(f->d_touched + a, 0, b - a, s);
        return e == hipSuccess ? 0 : fail("%s: clearing marks: %s (%d)", what, hipGetErrorString(e), (int)e);
    });
    auto copy_slots = [&](uint32_t a, uint32_t b) {
        const hipError_t e = hipMemcpyAsync(f->d_slots + a, f->h_slots + a, (size_t)(b - a) * sizeof(FlowSlot), hipMemcpyHostToDevice, s);
        return e == hipSuccess ? 0 : fail("%s: H2D slots: %s (%d)", what, hipGetErrorString(e), (int)e);
    };
    if (rc == 0) rc = whole ? copy_slots(0, f->t->slots()) : for_runs(dirty.idx, copy_slots);
    const hipError_t e = hipStreamSynchronize(s);   // also after a failed copy: none reads the mirror after the return
    if (rc != 0) return -1;   // the mirror is ahead of the device: the next update copies everything (resync)
    if (e != hipSuccess) return fail("%s: hipStreamSynchronize: %s (%d)", what, hipGetErrorString(e), (int)e);
    f->resync = false;
    return 0;
}

// The segment / datagram build of host memory (vpcsum_ctx_build_tcp_frames, vpcsum_ctx_build_udp_frames):
// frames written in place into a registered destination, the payloads read in place from a registered
// source or staged as one span.  Always launched (the service grid has no build), on the slot's one
// stream.  Rec: vpcsum_tcpseg_t or vpcsum_udpdg_t, both 32 B, whose copy lies in the slot's one pinned
// record buffer (h_tseg); `launch`: the kernel's, on the device addresses.
template <class Rec, class Launch>
static int ctx_build_frames(vpcsum_ctx_t* c, const char* what, const char* launch_what, uint8_t* h_dst, uint64_t dst_len,
                            const uint8_t* h_src, uint64_t src_len, const vpcsum_tcphdr_t* h_hdr, uint32_t n_hdr,
                            const Rec* h_rec, uint32_t n, uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status,
                            uint64_t* ticket, Launch launch) {
    static_assert(sizeof(Rec) == sizeof(vpcsum_tcpseg_t) && alignof(Rec) == alignof(vpcsum_tcpseg_t), "one record buffer for both");
    if (!c || !ticket) return fail("%s: NULL context or ticket", what);
    if (n > c->max_pkts) return fail("%s: %u records > capacity %u", what, n, c->max_pkts);
    if (n_hdr > c->max_pkts) return fail("%s: %u templates > capacity %u", what, n_hdr, c->max_pkts);
    if (n && (!h_dst || !h_rec || !h_frame_len || (!h_hdr && n_hdr) || (!h_src && src_len)))
        return fail("%s: NULL destination, source, templates, records or frame lengths", what);
    std::lock_guard<std::mutex> lk(c->mu);
    VPC_ON_DEVICE(c->device);
    uint8_t* base = n ? mapped_dev(c, h_dst, dst_len) : nullptr;
    if (n && !base) return fail("%s: the destination must be registered (vpcsum_ctx_register_arena)", what);
    // the source: read in place when registered, else the span of the payloads that lie inside it
    const uint8_t* src_dev = n && src_len ? mapped_dev(c, h_src, src_len) : nullptr;
    const bool staged = n && src_len && !src_dev;
    TcpPayloadSpan sp = {0, 0};
    if (staged && !tcp_build_payload_span(h_rec, n, src_len, c->max_arena, &sp))
        return fail("%s: the payloads span %llu bytes > capacity %llu", what, (unsigned long long)sp.len,
                    (unsigned long long)c->max_arena);
    Batch b;
    Slot* slot = slot_acquire(c, &b.ticket);
    if (!slot) return -1;
    Slot& s = *slot;
    b.n = n;
    b.zero_copy = true;   // the frames are written in place through the destination's mapping
    if (n) {
        // records, templates and frame lengths: pinned
        if (slot_scratch(c, what, s.h_tseg, s.h_thdr, s.h_tlen) != 0) return -1;
        b.hand_back({status_of(c, s, false, h_status, n), {h_frame_len, s.h_tlen.p, (size_t)n * 4}, out_of(c, s, false, h_out, n)});
        memcpy(s.h_tseg.p, h_rec, (size_t)n * sizeof(Rec));
        if (n_hdr) memcpy(s.h_thdr.p, h_hdr, (size_t)n_hdr * sizeof(vpcsum_tcphdr_t));
        if (staged) {
            // the library's copy of the records names the staged span
            tcp_build_rebase_payloads(reinterpret_cast<Rec*>(s.h_tseg.p), n, src_len, sp.lo);
            if (sp.len) memcpy(s.h_arena.p, h_src + sp.lo, sp.len);   // pageable -> pinned staging
            if (stage_frames_up(s, sp.len) != 0) return -1;
        }
        VPC_CHECK(launch(base, dst_len, staged ? s.d_arena.p : src_dev, staged ? sp.len : src_len, s.h_thdr.dev, n_hdr,
                         reinterpret_cast<const Rec*>(s.h_tseg.dev), n, s.h_tlen.dev, h_out ? s.h_out.dev : nullptr, s.h_status.dev,
                         s.stream),
                  launch_what);
    }
    return slot_commit(s, b, ticket);
}

// The TCP / UDP receive of host memory (vpcsum_ctx_recv_tcp_frames, vpcsum_ctx_recv_udp_frames):
// payloads written in place into a registered destination, the frames read in place from a registered
// arena or staged by vpcsum_ctx_submit's plan.  Always launched, on the slot's one stream; descriptors,
// records and results in mapped pinned memory.  Rec: vpcsum_tcprx_t or vpcsum_udprx_t, both 16 B, whose
// copy lies in the slot's one pinned record buffer (h_trx); `launch`: the kernel's, on the device addresses.
template <class Rec, class Launch>
static int ctx_recv_frames(vpcsum_ctx_t* c, const char* what, const char* launch_what, const uint8_t* h_arena, uint64_t arena_len,
                           const vpcsum_desc_t* h_desc, const Rec* h_rx, uint32_t n, uint8_t* h_dst, uint64_t dst_len,
                           uint32_t* h_stored, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket, Launch launch) {
    static_assert(sizeof(Rec) == sizeof(vpcsum_tcprx_t) && alignof(Rec) == alignof(vpcsum_tcprx_t), "one record buffer for both");
    if (desc_args(c, what, "arena, descriptors or records", h_arena, h_desc, h_rx, n, ticket) != 0) return -1;
    if (n && (!h_stored || (!h_dst && dst_len))) return fail("%s: NULL destination or stored counts", what);
    return desc_entry(c, const_cast<uint8_t*>(h_arena), arena_len, h_desc, n, VPCSUM_MODE_VERIFY,
                      [&](Slot& s, Batch& b, const BatchSpan& sp, uint8_t* base) {
        uint8_t* dst_dev = n && dst_len ? mapped_dev(c, h_dst, dst_len) : nullptr;
        if (n && dst_len && !dst_dev) return fail("%s: the destination must be registered (vpcsum_ctx_register_arena)", what);
        b.user_arena = nullptr;   // nothing goes back into the frames
        b.user_desc = nullptr;
        b.zero_copy = true;       // the payloads are written in place through the destination's mapping
        if (n) {
            if (slot_scratch(c, what, s.h_trx, s.h_tlen) != 0) return -1;
            b.hand_back({status_of(c, s, false, h_status, n), {h_stored, s.h_tlen.p, (size_t)n * 4}, out_of(c, s, false, h_out, n)});
            memcpy(s.h_trx.p, h_rx, (size_t)n * sizeof(Rec));
            uint64_t dev_len = arena_len;
            if (base) {
                memcpy(s.h_desc.p, h_desc, (size_t)n * sizeof(vpcsum_desc_t));
            } else {
                if (stage_desc_frames(c, s, what, h_arena, arena_len, h_desc, n, sp, &dev_len) != 0) return -1;
                if (stage_frames_up(s, dev_len) != 0) return -1;
            }
            VPC_CHECK(launch(base ? base : s.d_arena.p, dev_len, s.h_desc.dev, reinterpret_cast<const Rec*>(s.h_trx.dev), n,
                             dst_dev, dst_len, s.h_tlen.dev,
                             h_out ? s.h_out.dev : nullptr, s.h_status.dev, s.stream),
                      launch_what);
        }
        return slot_commit(s, b, ticket);
    });
}

// The ICMP replies of host memory (vpcsum_ctx_reply_icmp_frames): the source by ctx_recv_frames' plan
// (read in place from a registered arena, else staged as vpcsum_ctx_submit stages it), the destination
// by ctx_build_frames' (written in place, registered).  The 24-B records lie in the slot's pinned
// build-record buffer (h_tseg, 32 B per packet), the templates in h_thdr, the frame lengths in h_tlen
// and the replies' sums in h_port.
static int ctx_reply_icmp(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                          const vpcsum_icmphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_icmprp_t* h_rp, uint32_t n, uint8_t* h_dst,
                          uint64_t dst_len, uint32_t* h_frame_len, uint32_t* h_csum, uint32_t* h_out, uint8_t* h_status,
                          uint64_t* ticket) {
    static_assert(sizeof(vpcsum_icmprp_t) <= sizeof(vpcsum_tcpseg_t) && alignof(vpcsum_icmprp_t) <= alignof(vpcsum_tcpseg_t),
                  "the records fit the build-record buffer");
    const char* what = "vpcsum_ctx_reply_icmp_frames";
    if (desc_args(c, what, "arena, descriptors or records", h_arena, h_desc, h_rp, n, ticket) != 0) return -1;
    if (n_hdr > c->max_pkts) return fail("%s: %u templates > capacity %u", what, n_hdr, c->max_pkts);
    if (n && (!h_dst || !h_frame_len || (!h_hdr && n_hdr))) return fail("%s: NULL destination, templates or frame lengths", what);
    return desc_entry(c, const_cast<uint8_t*>(h_arena), arena_len, h_desc, n, VPCSUM_MODE_VERIFY,
                      [&](Slot& s, Batch& b, const BatchSpan& sp, uint8_t* base) {
        uint8_t* dst_dev = n ? mapped_dev(c, h_dst, dst_len) : nullptr;
        if (n && !dst_dev) return fail("%s: the destination must be registered (vpcsum_ctx_register_arena)", what);
        b.user_arena = nullptr;   // nothing goes back into the requests
        b.user_desc = nullptr;
        b.zero_copy = true;       // the replies are written in place through the destination's mapping
        if (n) {
            if (slot_scratch(c, what, s.h_tseg, s.h_thdr, s.h_tlen, s.h_port) != 0) return -1;
            b.hand_back({status_of(c, s, false, h_status, n), {h_frame_len, s.h_tlen.p, (size_t)n * 4},
                         {h_csum, s.h_port.p, (size_t)n * 4}, out_of(c, s, false, h_out, n)});
            memcpy(s.h_tseg.p, h_rp, (size_t)n * sizeof(vpcsum_icmprp_t));
            if (n_hdr) memcpy(s.h_thdr.p, h_hdr, (size_t)n_hdr * sizeof(vpcsum_icmphdr_t));
            uint64_t dev_len = arena_len;
            if (base) {
                memcpy(s.h_desc.p, h_desc, (size_t)n * sizeof(vpcsum_desc_t));
            } else {
                if (stage_desc_frames(c, s, what, h_arena, arena_len, h_desc, n, sp, &dev_len) != 0) return -1;
                if (stage_frames_up(s, dev_len) != 0) return -1;
            }
            VPC_CHECK(launch_icmp_reply(base ? base : s.d_arena.p, dev_len, s.h_desc.dev, s.h_thdr.dev, n_hdr,
                                        reinterpret_cast<const vpcsum_icmprp_t*>(s.h_tseg.dev), n, dst_dev, dst_len, s.h_tlen.dev,
                                        h_csum ? s.h_port.dev : nullptr, h_out ? s.h_out.dev : nullptr, s.h_status.dev, s.stream),
                      "ICMP reply launch");
        }
        return slot_commit(s, b, ticket);
    });
}

extern "C" {

int vpcsum_flowtab_create(int device, uint32_t max_flows, vpcsum_flowtab_t** out) {
    try {
        if (!out) return fail("vpcsum_flowtab_create: out is NULL");
        if (max_flows == 0 || max_flows > (1u << 24)) return fail("vpcsum_flowtab_create: max_flows %u outside 1..2^24", max_flows);
        VPC_ON_DEVICE(device);
        vpcsum_flowtab* f = new vpcsum_flowtab();
        f->device = device;
        f->max_flows = max_flows;
        const size_t bytes = (size_t)FlowTable::slots_for(max_flows) * sizeof(FlowSlot);
        hipError_t e = hipSuccess;
        if ((e = hipHostMalloc((void**)&f->h_slots, bytes, 0)) != hipSuccess ||
            (e = hipMalloc((void**)&f->d_slots, bytes)) != hipSuccess ||
            (e = hipMalloc((void**)&f->d_touched, max_flows)) != hipSuccess ||
            (e = hipHostMalloc((void**)&f->h_touched, max_flows, 0)) != hipSuccess ||
            (e = hipMemset(f->d_slots, 0, bytes)) != hipSuccess || (e = hipMemset(f->d_touched, 0, max_flows)) != hipSuccess ||
            (e = hipDeviceSynchronize()) != hipSuccess) {
            flowtab_free(f);
            return hipfail(e, "vpcsum_flowtab_create allocation");
        }
        memset((void*)f->h_slots, 0, bytes);
        try {
            f->t.reset(new FlowTable(max_flows, f->h_slots));
        } catch (...) {
            flowtab_free(f);
            throw;
        }
        *out = f;
        return 0;
    } VPC_CATCH("vpcsum_flowtab_create")
}

int vpcsum_flowtab_destroy(vpcsum_flowtab_t* f) {
    try {
        if (!f) return 0;
        DeviceScope on_dev(f->device);
        (void)hipDeviceSynchronize();   // lookups still reading the table finish first
        flowtab_free(f);
        return 0;
    } VPC_CATCH("vpcsum_flowtab_destroy")
}

int vpcsum_flowtab_update(vpcsum_flowtab_t* f, const vpcsum_tuple_t* h_del, uint32_t n_del, const vpcsum_flow_t* h_add,
                          uint32_t n_add, void* stream) {
    try {
        if (!f) return fail("vpcsum_flowtab_update: NULL table");
        if ((n_del && !h_del) || (n_add && !h_add)) return fail("vpcsum_flowtab_update: NULL keys or flows");
        std::lock_guard<std::mutex> lk(f->mu);
        VPC_ON_DEVICE(f->device);
        std::string why;
        if (!f->t->validate(h_del, n_del, h_add, n_add, &why)) return fail("vpcsum_flowtab_update: %s", why.c_str());
        // room for the bookkeeping before the table changes: nothing below refuses (validated) or
        // allocates (FlowTable, FlowDirty), so the mirror is never left half changed
        FlowDirty dirty((size_t)n_del * 4 + n_add + 16);
        std::vector<uint32_t> freed;
        freed.reserve(n_del);
        for (uint32_t i = 0; i < n_del; ++i) {
            const int64_t id = f->t->erase(h_del[i], &dirty);
            if (id >= 0) freed.push_back((uint32_t)id);
        }
        for (uint32_t i = 0; i < n_add; ++i) (void)f->t->insert(h_add[i], &dirty);
        return flowtab_push(f, dirty, freed, (hipStream_t)stream, "vpcsum_flowtab_update");
    } VPC_CATCH("vpcsum_flowtab_update")
}

int vpcsum_flowtab_info(vpcsum_flowtab_t* f, uint32_t* slots, uint32_t* flows, uint32_t* max_probe) {
    try {
        if (!f) return fail("vpcsum_flowtab_info: NULL table");
        std::lock_guard<std::mutex> lk(f->mu);
        if (slots) *slots = f->t->slots();
        if (flows) *flows = f->t->flows();
        if (max_probe) *max_probe = f->t->max_probe();
        return 0;
    } VPC_CATCH("vpcsum_flowtab_info")
}

int vpcsum_flow_hash(const vpcsum_tuple_t* key, uint64_t* out) {
    try {
        if (!key || !out) return fail("vpcsum_flow_hash: NULL argument");
        *out = flow_hash(*key);
        return 0;
    } VPC_CATCH("vpcsum_flow_hash")
}

int vpcsum_flow_lookup_async(vpcsum_flowtab_t* f, const vpcsum_tuple_t* d_tuples, uint32_t n, vpcsum_nat_t* d_rw,
                             uint8_t* d_verdict, void* stream) {
    try {
        return flow_lookup_async("vpcsum_flow_lookup_async", false, f, d_tuples, n, d_rw, d_verdict, nullptr, stream);
    } VPC_CATCH("vpcsum_flow_lookup_async")
}

int vpcsum_flowtab_set_fastpath(vpcsum_flowtab_t* f, const vpcsum_tuple_t* h_keys, const vpcsum_fastpath_t* h_fp, uint32_t n,
                                uint32_t* n_missing, void* stream) {
    try {
        if (!f) return fail("vpcsum_flowtab_set_fastpath: NULL table");
        if (n && (!h_keys || !h_fp)) return fail("vpcsum_flowtab_set_fastpath: NULL keys or Fastpath records");
        std::lock_guard<std::mutex> lk(f->mu);
        VPC_ON_DEVICE(f->device);
        // every key checked, and the bookkeeping's room made, before the table changes
        for (uint32_t i = 0; i < n; ++i)
            if (const char* r = flow_key_refusal(h_keys[i])) return fail("vpcsum_flowtab_set_fastpath: key %u: %s", i, r);
        FlowDirty dirty((size_t)n + 16);
        std::vector<uint32_t> none;
        uint32_t missing = 0;
        for (uint32_t i = 0; i < n; ++i) missing += f->t->set_fastpath(h_keys[i], h_fp[i], &dirty) == 0 ? 1u : 0u;
        if (n_missing) *n_missing = missing;
        return flowtab_push(f, dirty, none, (hipStream_t)stream, "vpcsum_flowtab_set_fastpath");
    } VPC_CATCH("vpcsum_flowtab_set_fastpath")
}

int vpcsum_flow_lookup_fp_async(vpcsum_flowtab_t* f, const vpcsum_tuple_t* d_tuples, uint32_t n, vpcsum_nat_t* d_rw,
                                uint8_t* d_verdict, vpcsum_fastpath_t* d_fp, void* stream) {
    try {
        return flow_lookup_async("vpcsum_flow_lookup_fp_async", true, f, d_tuples, n, d_rw, d_verdict, d_fp, stream);
    } VPC_CATCH("vpcsum_flow_lookup_fp_async")
}

int vpcsum_l2_forward_async(uint8_t* d_arena, uint64_t arena_len, const uint64_t* d_frame_off, const uint32_t* d_frame_len,
                            const uint8_t* d_verdict, const uint8_t* d_status, const vpcsum_fastpath_t* d_fp, uint32_t n,
                            uint32_t* d_port, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena || !d_frame_off || !d_frame_len || !d_verdict || !d_status || !d_fp || !d_port)
            return fail("vpcsum_l2_forward_async: NULL argument");
        if ((uintptr_t)d_frame_off & 7) return fail("vpcsum_l2_forward_async: frame offsets not 8-byte aligned");
        if (((uintptr_t)d_frame_len | (uintptr_t)d_fp | (uintptr_t)d_port) & 3)
            return fail("vpcsum_l2_forward_async: frame lengths / Fastpath records / ports not 4-byte aligned");
        if (n > (1u << 28)) return fail("vpcsum_l2_forward_async: %u frames > 2^28", n);
        VPC_CHECK(launch_l2_forward(d_arena, arena_len, d_frame_off, d_frame_len, d_verdict, d_status, d_fp, n, d_port,
                                    (hipStream_t)stream),
                  "L2 forward launch");
        return 0;
    } VPC_CATCH("vpcsum_l2_forward_async")
}

int vpcsum_tcp_build_async(uint8_t* d_dst, uint64_t dst_len, const uint8_t* d_src, uint64_t src_len,
                           const vpcsum_tcphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_tcpseg_t* d_seg, uint32_t n,
                           uint32_t* d_frame_len, uint32_t* d_out, uint8_t* d_status, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_dst) return fail("vpcsum_tcp_build_async: NULL destination arena");
        if (!d_src && src_len) return fail("vpcsum_tcp_build_async: NULL source arena");
        if (!d_hdr && n_hdr) return fail("vpcsum_tcp_build_async: NULL templates");
        if (!d_seg) return fail("vpcsum_tcp_build_async: NULL records");
        if (!d_frame_len) return fail("vpcsum_tcp_build_async: NULL frame lengths");
        if ((uintptr_t)d_seg & 7) return fail("vpcsum_tcp_build_async: records not 8-byte aligned");
        if ((uintptr_t)d_hdr & 3) return fail("vpcsum_tcp_build_async: templates not 4-byte aligned");
        if ((uintptr_t)d_frame_len & 3) return fail("vpcsum_tcp_build_async: frame lengths not 4-byte aligned");
        if ((uintptr_t)d_out & 3) return fail("vpcsum_tcp_build_async: out words not 4-byte aligned");
        if (n > (1u << 28)) return fail("vpcsum_tcp_build_async: %u records > 2^28", n);
        VPC_CHECK(launch_tcp_build(d_dst, dst_len, d_src, src_len, d_hdr, n_hdr, d_seg, n, d_frame_len, d_out, d_status,
                                   (hipStream_t)stream),
                  "TCP build launch");
        return 0;
    } VPC_CATCH("vpcsum_tcp_build_async")
}

int vpcsum_tcp_build_bursts_async(uint8_t* d_dst, uint64_t dst_len, const uint8_t* d_src, uint64_t src_len,
                                  const vpcsum_tcphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_tcpburst_t* d_burst,
                                  uint32_t n_bursts, const uint64_t* d_frame_off, uint32_t n_frames, uint32_t frame_cap,
                                  uint32_t* d_frame_len, uint32_t* d_out, uint8_t* d_status, void* stream) {
    try {
        if (n_frames == 0) return 0;
        if (!d_dst) return fail("vpcsum_tcp_build_bursts_async: NULL destination arena");
        if (!d_src && src_len) return fail("vpcsum_tcp_build_bursts_async: NULL source arena");
        if (!d_hdr && n_hdr) return fail("vpcsum_tcp_build_bursts_async: NULL templates");
        if (!d_burst && n_bursts) return fail("vpcsum_tcp_build_bursts_async: NULL bursts");
        if (!d_frame_off) return fail("vpcsum_tcp_build_bursts_async: NULL frame offsets");
        if (!d_frame_len) return fail("vpcsum_tcp_build_bursts_async: NULL frame lengths");
        if ((uintptr_t)d_burst & 7) return fail("vpcsum_tcp_build_bursts_async: bursts not 8-byte aligned");
        if ((uintptr_t)d_frame_off & 7) return fail("vpcsum_tcp_build_bursts_async: frame offsets not 8-byte aligned");
        if ((uintptr_t)d_hdr & 3) return fail("vpcsum_tcp_build_bursts_async: templates not 4-byte aligned");
        if ((uintptr_t)d_frame_len & 3) return fail("vpcsum_tcp_build_bursts_async: frame lengths not 4-byte aligned");
        if ((uintptr_t)d_out & 3) return fail("vpcsum_tcp_build_bursts_async: out words not 4-byte aligned");
        if (n_frames > (1u << 28)) return fail("vpcsum_tcp_build_bursts_async: %u frames > 2^28", n_frames);
        if (n_bursts > (1u << 28)) return fail("vpcsum_tcp_build_bursts_async: %u bursts > 2^28", n_bursts);
        VPC_CHECK(launch_tcp_build_bursts(d_dst, dst_len, d_src, src_len, d_hdr, n_hdr, d_burst, n_bursts, d_frame_off, n_frames,
                                          frame_cap, d_frame_len, d_out, d_status, (hipStream_t)stream),
                  "TCP burst build launch");
        return 0;
    } VPC_CATCH("vpcsum_tcp_build_bursts_async")
}

int vpcsum_tcp_recv_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const vpcsum_tcprx_t* d_rx,
                          uint32_t n, uint8_t* d_dst, uint64_t dst_len, uint32_t* d_stored, uint32_t* d_out, uint8_t* d_status,
                          void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena && arena_len) return fail("vpcsum_tcp_recv_async: NULL arena");
        if (!d_desc || !d_rx) return fail("vpcsum_tcp_recv_async: NULL descriptors or records");
        if (!d_dst && dst_len) return fail("vpcsum_tcp_recv_async: NULL destination arena");
        if (!d_stored) return fail("vpcsum_tcp_recv_async: NULL stored counts");
        if (((uintptr_t)d_desc | (uintptr_t)d_rx) & 7) return fail("vpcsum_tcp_recv_async: descriptors or records not 8-byte aligned");
        if ((uintptr_t)d_stored & 3) return fail("vpcsum_tcp_recv_async: stored counts not 4-byte aligned");
        if ((uintptr_t)d_out & 3) return fail("vpcsum_tcp_recv_async: out words not 4-byte aligned");
        if (n > (1u << 28)) return fail("vpcsum_tcp_recv_async: %u records > 2^28", n);
        VPC_CHECK(launch_tcp_recv(d_arena, arena_len, d_desc, d_rx, n, d_dst, dst_len, d_stored, d_out, d_status,
                                  (hipStream_t)stream),
                  "TCP receive launch");
        return 0;
    } VPC_CATCH("vpcsum_tcp_recv_async")
}

int vpcsum_tcp_digest_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, uint32_t n,
                            vpcsum_tcpinfo_t* d_info, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena && arena_len) return fail("vpcsum_tcp_digest_async: NULL arena");
        if (!d_desc || !d_info) return fail("vpcsum_tcp_digest_async: NULL descriptors or records");
        if ((uintptr_t)d_desc & 7) return fail("vpcsum_tcp_digest_async: descriptors not 8-byte aligned");
        if ((uintptr_t)d_info & 15) return fail("vpcsum_tcp_digest_async: records not 16-byte aligned");
        VPC_CHECK(launch_tcp_digest(d_arena, arena_len, d_desc, n, d_info, (hipStream_t)stream), "TCP digest launch");
        return 0;
    } VPC_CATCH("vpcsum_tcp_digest_async")
}

int vpcsum_udp_build_async(uint8_t* d_dst, uint64_t dst_len, const uint8_t* d_src, uint64_t src_len,
                           const vpcsum_udphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_udpdg_t* d_dg, uint32_t n,
                           uint32_t* d_frame_len, uint32_t* d_out, uint8_t* d_status, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_dst) return fail("vpcsum_udp_build_async: NULL destination arena");
        if (!d_src && src_len) return fail("vpcsum_udp_build_async: NULL source arena");
        if (!d_hdr && n_hdr) return fail("vpcsum_udp_build_async: NULL templates");
        if (!d_dg) return fail("vpcsum_udp_build_async: NULL records");
        if (!d_frame_len) return fail("vpcsum_udp_build_async: NULL frame lengths");
        if ((uintptr_t)d_dg & 7) return fail("vpcsum_udp_build_async: records not 8-byte aligned");
        if ((uintptr_t)d_hdr & 3) return fail("vpcsum_udp_build_async: templates not 4-byte aligned");
        if ((uintptr_t)d_frame_len & 3) return fail("vpcsum_udp_build_async: frame lengths not 4-byte aligned");
        if ((uintptr_t)d_out & 3) return fail("vpcsum_udp_build_async: out words not 4-byte aligned");
        if (n > (1u << 28)) return fail("vpcsum_udp_build_async: %u records > 2^28", n);
        VPC_CHECK(launch_udp_build(d_dst, dst_len, d_src, src_len, d_hdr, n_hdr, d_dg, n, d_frame_len, d_out, d_status,
                                   (hipStream_t)stream),
                  "UDP build launch");
        return 0;
    } VPC_CATCH("vpcsum_udp_build_async")
}

int vpcsum_udp_recv_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const vpcsum_udprx_t* d_rx,
                          uint32_t n, uint8_t* d_dst, uint64_t dst_len, uint32_t* d_stored, uint32_t* d_out, uint8_t* d_status,
                          void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena && arena_len) return fail("vpcsum_udp_recv_async: NULL arena");
        if (!d_desc || !d_rx) return fail("vpcsum_udp_recv_async: NULL descriptors or records");
        if (!d_dst && dst_len) return fail("vpcsum_udp_recv_async: NULL destination arena");
        if (!d_stored) return fail("vpcsum_udp_recv_async: NULL stored counts");
        if (((uintptr_t)d_desc | (uintptr_t)d_rx) & 7) return fail("vpcsum_udp_recv_async: descriptors or records not 8-byte aligned");
        if ((uintptr_t)d_stored & 3) return fail("vpcsum_udp_recv_async: stored counts not 4-byte aligned");
        if ((uintptr_t)d_out & 3) return fail("vpcsum_udp_recv_async: out words not 4-byte aligned");
        if (n > (1u << 28)) return fail("vpcsum_udp_recv_async: %u records > 2^28", n);
        VPC_CHECK(launch_udp_recv(d_arena, arena_len, d_desc, d_rx, n, d_dst, dst_len, d_stored, d_out, d_status,
                                  (hipStream_t)stream),
                  "UDP receive launch");
        return 0;
    } VPC_CATCH("vpcsum_udp_recv_async")
}

int vpcsum_icmp_reply_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const vpcsum_icmphdr_t* d_hdr,
                            uint32_t n_hdr, const vpcsum_icmprp_t* d_rp, uint32_t n, uint8_t* d_dst, uint64_t dst_len,
                            uint32_t* d_frame_len, uint32_t* d_csum, uint32_t* d_out, uint8_t* d_status, void* stream) {
    try {
        if (n == 0) return 0;
        if (!d_arena && arena_len) return fail("vpcsum_icmp_reply_async: NULL arena");
        if (!d_desc || !d_rp) return fail("vpcsum_icmp_reply_async: NULL descriptors or records");
        if (!d_hdr && n_hdr) return fail("vpcsum_icmp_reply_async: NULL templates");
        if (!d_dst) return fail("vpcsum_icmp_reply_async: NULL destination arena");
        if (!d_frame_len) return fail("vpcsum_icmp_reply_async: NULL frame lengths");
        if (((uintptr_t)d_desc | (uintptr_t)d_rp) & 7) return fail("vpcsum_icmp_reply_async: descriptors or records not 8-byte aligned");
        if ((uintptr_t)d_hdr & 3) return fail("vpcsum_icmp_reply_async: templates not 4-byte aligned");
        if ((uintptr_t)d_frame_len & 3) return fail("vpcsum_icmp_reply_async: frame lengths not 4-byte aligned");
        if (((uintptr_t)d_csum | (uintptr_t)d_out) & 3) return fail("vpcsum_icmp_reply_async: sum or out words not 4-byte aligned");
        if (n > (1u << 28)) return fail("vpcsum_icmp_reply_async: %u records > 2^28", n);
        VPC_CHECK(launch_icmp_reply(d_arena, arena_len, d_desc, d_hdr, n_hdr, d_rp, n, d_dst, dst_len, d_frame_len, d_csum, d_out,
                                    d_status, (hipStream_t)stream),
                  "ICMP reply launch");
        return 0;
    } VPC_CATCH("vpcsum_icmp_reply_async")
}

int vpcsum_flowtab_collect(vpcsum_flowtab_t* f, uint64_t* h_cookies, uint32_t cap, uint32_t* n_out, void* stream) {
    try {
        if (!f || !n_out) return fail("vpcsum_flowtab_collect: NULL table or count");
        if (cap && !h_cookies) return fail("vpcsum_flowtab_collect: NULL cookies");
        std::lock_guard<std::mutex> lk(f->mu);
        VPC_ON_DEVICE(f->device);
        hipStream_t s = (hipStream_t)stream;
        VPC_CHECK(hipMemcpyAsync(f->h_touched, f->d_touched, f->max_flows, hipMemcpyDeviceToHost, s), "vpcsum_flowtab_collect: D2H marks");
        VPC_CHECK(hipStreamSynchronize(s), "vpcsum_flowtab_collect: hipStreamSynchronize");
        uint32_t cnt = 0;
        for (uint32_t id = 0; id < f->max_flows; ++id) cnt += (f->h_touched[id] && f->t->live(id)) ? 1u : 0u;
        *n_out = cnt;
        if (cnt > cap) return 0;   // nothing cleared: the caller comes back with room
        uint32_t k = 0;
        for (uint32_t id = 0; id < f->max_flows; ++id)
            if (f->h_touched[id] && f->t->live(id)) h_cookies[k++] = f->t->cookie(id);
        if (cnt) VPC_CHECK(hipMemsetAsync(f->d_touched, 0, f->max_flows, s), "vpcsum_flowtab_collect: clearing marks");
        return 0;
    } VPC_CATCH("vpcsum_flowtab_collect")
}

// vpcsum_ctx_nat_flow_frames (h_port NULL, forward false) / vpcsum_ctx_nat_flow_forward_frames
static int ctx_nat_flow_frames(vpcsum_ctx_t* c, vpcsum_flowtab_t* f, uint8_t* h_arena, uint64_t arena_len,
                               const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n, uint8_t* h_status,
                               uint8_t* h_verdict, uint32_t* h_port, bool forward, uint32_t nat_mode, uint64_t* ticket,
                               const char* what) {
    if (!f) return fail("%s: NULL flow table", what);
    if (c && f->device != c->device)
        return fail("%s: the flow table lives on device %d, the context on device %d", what, f->device, c->device);
    if (nat_mode & ~kNatCtxModeAccept) return fail("%s: bad nat_mode 0x%x", what, nat_mode);
    if (n && !h_verdict) return fail("%s: NULL verdicts", what);
    if (n && forward && !h_port) return fail("%s: NULL ports", what);
    // the service grid has no lookup: the batch is launched whatever its size (may_svc false)
    return frames_entry(c, what, "arena, frame table or status", h_arena, arena_len, h_frame_off, h_frame_len, h_status, n,
                        ticket, [&](Slot& s, Batch b, uint8_t* base, bool) {
        b.mode = nat_mode;   // zero-copy: the frames are rewritten where they lie
        if (n) {
            // per-packet scratch of the chain: entries and tuples on the device, verdicts in pinned
            // memory; a forwarding batch: Fastpath records on the device, ports in pinned memory
            if (slot_scratch(c, what, s.h_rw, s.d_rw, s.d_tu, s.h_verdict) != 0) return -1;
            if (forward && slot_scratch(c, what, s.d_fp, s.h_port) != 0) return -1;
            b.hand_back({status_of(c, s, false, h_status, n), {h_verdict, s.h_verdict.p, n},
                         {forward ? h_port : nullptr, s.h_port.p, (size_t)n * 4}});
            // parse -> tuples -> lookup -> entries -> rewrite (-> L2 write), one stream; the parse's
            // status bytes are not needed: a refused frame's descriptor is all zeros, which the
            // rewrite refuses (S_BAD_DESC, nothing written)
            VPC_CHECK(launch_parse_ether(base, arena_len, s.h_foff.dev, s.h_flen.dev, n, VPCSUM_F_IP | VPCSUM_F_L4, s.d_desc.p,
                                         nullptr, s.d_tu.p, s.stream),
                      "parse launch");
            if (flow_lookup(f, s.d_tu.p, n, s.d_rw.p, s.h_verdict.dev, forward ? s.d_fp.p : nullptr, s.stream) != 0) return -1;
            if (nat_run(base, arena_len, s.d_desc.p, s.d_rw.p, 1, n, s.h_status.dev, nat_mode, s.stream) != 0) return -1;
            // the rewrite's status says which HIT frames are complete: those get their flow's addresses
            if (forward)
                VPC_CHECK(launch_l2_forward(base, arena_len, s.h_foff.dev, s.h_flen.dev, s.h_verdict.dev, s.h_status.dev, s.d_fp.p,
                                            n, s.h_port.dev, s.stream),
                          "L2 forward launch");
        }
        return slot_commit(s, b, ticket);
    }, false);
}

int vpcsum_ctx_nat_flow_frames(vpcsum_ctx_t* c, vpcsum_flowtab_t* f, uint8_t* h_arena, uint64_t arena_len,
                               const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n, uint8_t* h_status,
                               uint8_t* h_verdict, uint32_t nat_mode, uint64_t* ticket) {
    try {
        return ctx_nat_flow_frames(c, f, h_arena, arena_len, h_frame_off, h_frame_len, n, h_status, h_verdict, nullptr, false,
                                   nat_mode, ticket, "vpcsum_ctx_nat_flow_frames");
    } VPC_CATCH("vpcsum_ctx_nat_flow_frames")
}

int vpcsum_ctx_nat_flow_forward_frames(vpcsum_ctx_t* c, vpcsum_flowtab_t* f, uint8_t* h_arena, uint64_t arena_len,
                                       const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n,
                                       uint8_t* h_status, uint8_t* h_verdict, uint32_t* h_port, uint32_t nat_mode,
                                       uint64_t* ticket) {
    try {
        return ctx_nat_flow_frames(c, f, h_arena, arena_len, h_frame_off, h_frame_len, n, h_status, h_verdict, h_port, true,
                                   nat_mode, ticket, "vpcsum_ctx_nat_flow_forward_frames");
    } VPC_CATCH("vpcsum_ctx_nat_flow_forward_frames")
}

int vpcsum_ctx_build_tcp_frames(vpcsum_ctx_t* c, uint8_t* h_dst, uint64_t dst_len, const uint8_t* h_src, uint64_t src_len,
                                const vpcsum_tcphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_tcpseg_t* h_seg, uint32_t n,
                                uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket) {
    try {
        return ctx_build_frames(c, "vpcsum_ctx_build_tcp_frames", "TCP build launch", h_dst, dst_len, h_src, src_len, h_hdr, n_hdr,
                                h_seg, n, h_frame_len, h_out, h_status, ticket, launch_tcp_build);
    } VPC_CATCH("vpcsum_ctx_build_tcp_frames")
}

int vpcsum_ctx_build_udp_frames(vpcsum_ctx_t* c, uint8_t* h_dst, uint64_t dst_len, const uint8_t* h_src, uint64_t src_len,
                                const vpcsum_udphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_udpdg_t* h_dg, uint32_t n,
                                uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket) {
    try {
        return ctx_build_frames(c, "vpcsum_ctx_build_udp_frames", "UDP build launch", h_dst, dst_len, h_src, src_len, h_hdr, n_hdr,
                                h_dg, n, h_frame_len, h_out, h_status, ticket, launch_udp_build);
    } VPC_CATCH("vpcsum_ctx_build_udp_frames")
}

// The TCP send bursts of host memory: vpcsum_ctx_build_tcp_frames with bursts for records and the
// frame table beside them.  Always launched, on the slot's one stream.
int vpcsum_ctx_build_tcp_bursts(vpcsum_ctx_t* c, uint8_t* h_dst, uint64_t dst_len, const uint8_t* h_src, uint64_t src_len,
                                const vpcsum_tcphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_tcpburst_t* h_burst,
                                uint32_t n_bursts, const uint64_t* h_frame_off, uint32_t n_frames, uint32_t frame_cap,
                                uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket) {
    const char* what = "vpcsum_ctx_build_tcp_bursts";
    try {
        if (!c || !ticket) return fail("%s: NULL context or ticket", what);
        const uint32_t n = n_frames;
        if (n > c->max_pkts) return fail("%s: %u frames > capacity %u", what, n, c->max_pkts);
        if (n_bursts > c->max_pkts) return fail("%s: %u bursts > capacity %u", what, n_bursts, c->max_pkts);
        if (n_hdr > c->max_pkts) return fail("%s: %u templates > capacity %u", what, n_hdr, c->max_pkts);
        if (n && (!h_dst || !h_frame_off || !h_frame_len || (!h_burst && n_bursts) || (!h_hdr && n_hdr) || (!h_src && src_len)))
            return fail("%s: NULL destination, source, templates, bursts, frame offsets or frame lengths", what);
        std::lock_guard<std::mutex> lk(c->mu);
        VPC_ON_DEVICE(c->device);
        uint8_t* base = n ? mapped_dev(c, h_dst, dst_len) : nullptr;
        if (n && !base) return fail("%s: the destination must be registered (vpcsum_ctx_register_arena)", what);
        // the source: read in place when registered, else the span of the payloads that lie inside it
        const uint8_t* src_dev = n && src_len ? mapped_dev(c, h_src, src_len) : nullptr;
        const bool staged = n && src_len && !src_dev;
        TcpPayloadSpan sp = {0, 0};
        if (staged && !tcp_burst_payload_span(h_burst, n_bursts, src_len, c->max_arena, &sp))
            return fail("%s: the payloads span %llu bytes > capacity %llu", what, (unsigned long long)sp.len,
                        (unsigned long long)c->max_arena);
        Batch b;
        Slot* slot = slot_acquire(c, &b.ticket);
        if (!slot) return -1;
        Slot& s = *slot;
        b.n = n;
        b.zero_copy = true;   // the frames are written in place through the destination's mapping
        if (n) {
            // bursts, templates and frame lengths: pinned; the frame table in the slot's own
            if (slot_scratch(c, what, s.h_tburst, s.h_thdr, s.h_tlen) != 0) return -1;
            b.hand_back({status_of(c, s, false, h_status, n), {h_frame_len, s.h_tlen.p, (size_t)n * 4}, out_of(c, s, false, h_out, n)});
            memcpy(s.h_foff.p, h_frame_off, (size_t)n * 8);
            if (n_bursts) memcpy(s.h_tburst.p, h_burst, (size_t)n_bursts * sizeof(vpcsum_tcpburst_t));
            if (n_hdr) memcpy(s.h_thdr.p, h_hdr, (size_t)n_hdr * sizeof(vpcsum_tcphdr_t));
            if (staged) {
                // the library's copy of the bursts names the staged span
                tcp_burst_rebase_payloads(s.h_tburst.p, n_bursts, src_len, sp.lo);
                if (sp.len) memcpy(s.h_arena.p, h_src + sp.lo, sp.len);   // pageable -> pinned staging
                if (stage_frames_up(s, sp.len) != 0) return -1;
            }
            VPC_CHECK(launch_tcp_build_bursts(base, dst_len, staged ? s.d_arena.p : src_dev, staged ? sp.len : src_len,
                                              s.h_thdr.dev, n_hdr, s.h_tburst.dev, n_bursts, s.h_foff.dev, n, frame_cap,
                                              s.h_tlen.dev, h_out ? s.h_out.dev : nullptr, s.h_status.dev, s.stream),
                      "TCP burst build launch");
        }
        return slot_commit(s, b, ticket);
    } VPC_CATCH("vpcsum_ctx_build_tcp_bursts")
}

int vpcsum_ctx_recv_tcp_frames(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                               const vpcsum_tcprx_t* h_rx, uint32_t n, uint8_t* h_dst, uint64_t dst_len, uint32_t* h_stored,
                               uint32_t* h_out, uint8_t* h_status, uint64_t* ticket) {
    try {
        return ctx_recv_frames(c, "vpcsum_ctx_recv_tcp_frames", "TCP receive launch", h_arena, arena_len, h_desc, h_rx, n, h_dst,
                               dst_len, h_stored, h_out, h_status, ticket, launch_tcp_recv);
    } VPC_CATCH("vpcsum_ctx_recv_tcp_frames")
}

int vpcsum_ctx_recv_udp_frames(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                               const vpcsum_udprx_t* h_rx, uint32_t n, uint8_t* h_dst, uint64_t dst_len, uint32_t* h_stored,
                               uint32_t* h_out, uint8_t* h_status, uint64_t* ticket) {
    try {
        return ctx_recv_frames(c, "vpcsum_ctx_recv_udp_frames", "UDP receive launch", h_arena, arena_len, h_desc, h_rx, n, h_dst,
                               dst_len, h_stored, h_out, h_status, ticket, launch_udp_recv);
    } VPC_CATCH("vpcsum_ctx_recv_udp_frames")
}

int vpcsum_ctx_reply_icmp_frames(vpcsum_ctx_t* c, const uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                                 const vpcsum_icmphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_icmprp_t* h_rp, uint32_t n,
                                 uint8_t* h_dst, uint64_t dst_len, uint32_t* h_frame_len, uint32_t* h_csum, uint32_t* h_out,
                                 uint8_t* h_status, uint64_t* ticket) {
    try {
        return ctx_reply_icmp(c, h_arena, arena_len, h_desc, h_hdr, n_hdr, h_rp, n, h_dst, dst_len, h_frame_len, h_csum, h_out,
                              h_status, ticket);
    } VPC_CATCH("vpcsum_ctx_reply_icmp_frames")
}

int vpcsum_ctx_pipeline(vpcsum_ctx_t* c, uint8_t* h_arena, uint32_t stride, uint32_t copy_bytes,
                        const vpcsum_desc_t* h_desc, uint32_t n, uint32_t* h_out, uint32_t mode, uint32_t chunks) {
    try {
        if (!c || !h_arena || !h_desc || !h_out) return fail("vpcsum_ctx_pipeline: NULL argument");
        if (chunks == 0) chunks = 1;
        if (copy_bytes > stride) return fail("vpcsum_ctx_pipeline: copy_bytes > stride");
        if (mode & ~(VPCSUM_MODE_VERIFY | VPCSUM_MODE_WRITE)) return fail("vpcsum_ctx_pipeline: bad mode");
        std::lock_guard<std::mutex> lk(c->mu);
        VPC_ON_DEVICE(c->device);
        for (auto& s : c->slots)
            if (s.busy && slot_finish(c, s) != 0) return -1;
        const uint32_t per = (n + chunks - 1) / chunks;
        if (per > c->max_pkts || (uint64_t)per * stride > c->max_arena)
            return fail("vpcsum_ctx_pipeline: chunk of %u frames exceeds context capacity", per);
        const bool pinned = is_registered(c, h_arena, (uint64_t)n * stride);
        if (!pinned) return fail("vpcsum_ctx_pipeline: host arena must be registered (vpcsum_ctx_register_arena)");
        // MODE_WRITE: the kernels read the device copy and store the checksum fields straight into the
        // host frames through the registered arena's mapping (2-B posted PCIe writes), so the frames
        // need no copy back
        uint8_t* w = nullptr;
        if (mode & VPCSUM_MODE_WRITE) {
            w = mapped_dev(c, h_arena, (uint64_t)n * stride);
            if (!w) return fail("vpcsum_ctx_pipeline: MODE_WRITE needs the arena registered with this context");
        }
        const bool desc_pinned = is_registered(c, (const uint8_t*)h_desc, (uint64_t)n * sizeof(vpcsum_desc_t));
        const bool out_pinned = is_registered(c, (const uint8_t*)h_out, (uint64_t)n * 4);
        if (!desc_pinned || !out_pinned) return fail("vpcsum_ctx_pipeline: descriptors and out must be registered");
        // each chunk's device view starts at frame i0, and only the first copy_bytes of every frame
        // are copied: a descriptor must lie inside the copied part of a frame of its own chunk
        // (below the view it would address memory before the device slot)
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t i0 = (uint64_t)(i / per) * per;
            const uint64_t off = h_desc[i].l3_off;
            if (off < i0 * stride || off >= (uint64_t)n * stride || off % stride + h_desc[i].l3_len > copy_bytes)
                return fail("vpcsum_ctx_pipeline: descriptor %u [%llu, +%u) outside the copied frames", i,
                            (unsigned long long)off, (unsigned)h_desc[i].l3_len);
        }
        // a failure after some chunks were queued drains both streams before it returns: the queued
        // copies and in-place writes land in the caller's registered buffers
    #define VPC_CHECK_DRAIN(expr, what)                                                  \
        do {                                                                             \
            hipError_t e__ = (expr);                                                     \
            if (e__ != hipSuccess) {                                                     \
                const int rc__ = hipfail(e__, what);                                     \
                for (auto& q__ : c->slots) (void)hipStreamSynchronize(q__.stream);       \
                return rc__;                                                             \
            }                                                                            \
        } while (0)
        for (uint32_t k = 0; k < chunks; ++k) {
            const uint32_t i0 = k * per;
            if (i0 >= n) break;
            const uint32_t m = std::min(per, n - i0);
            Slot& s = c->slots[k & 1];
            // descriptors of this chunk address the device slot as frame (i - i0) * stride: the
            // caller's descriptors are relative to frame i0 once i0 * stride is subtracted
            VPC_CHECK_DRAIN(hipMemcpyAsync(s.d_desc.p, h_desc + i0, (size_t)m * sizeof(vpcsum_desc_t), hipMemcpyHostToDevice,
                                     s.stream),
                      "pipeline H2D desc");
            VPC_CHECK_DRAIN(hipMemcpy2DAsync(s.d_arena.p, stride, h_arena + (uint64_t)i0 * stride, stride, copy_bytes, m,
                                       hipMemcpyHostToDevice, s.stream),
                      "pipeline H2D frames");
            VPC_CHECK_DRAIN(launch_csum(s.d_arena.p - (uint64_t)i0 * stride, (uint64_t)(i0 + m) * stride, s.d_desc.p, m, s.d_out.p,
                                  nullptr, nullptr, (mode & VPCSUM_MODE_VERIFY) != 0, w, CsumTune{}, s.stream),
                      "pipeline launch");
            VPC_CHECK_DRAIN(hipMemcpyAsync(h_out + i0, s.d_out.p, (size_t)m * 4, hipMemcpyDeviceToHost, s.stream), "pipeline D2H");
        }
    #undef VPC_CHECK_DRAIN
        hipError_t es = hipSuccess;   // both streams are joined, the first error is reported
        for (auto& s : c->slots) {
            const hipError_t e2 = hipStreamSynchronize(s.stream);
            if (es == hipSuccess) es = e2;
        }
        VPC_CHECK(es, "pipeline sync");
        return 0;
    } VPC_CATCH("vpcsum_ctx_pipeline")
}

// ------------------------------------------------------------------------------------------
// Device groups (SURVEY.md §8(b) vpcsum_init(dev_mask), §8(e)): one context per GPU; a host batch
// is cut into contiguous descriptor ranges of nearly equal byte totals, one per GPU, each run by
// its own context (own streams, own staging); wait joins them.  No data crosses devices.
// ------------------------------------------------------------------------------------------
}  // extern "C"

struct vpcsum_group {
    std::vector<vpcsum_ctx*> ctx;
    struct Reg { uint8_t* host; uint8_t* key; };
    std::vector<Reg> reg;          // arenas the group registered: their page-lock references (portable
                                   // locks: every device maps them), one per arena
    uint64_t next_ticket = 1;
    struct Pending { uint64_t ticket = 0; std::vector<uint64_t> sub; };
    Pending slots[2];
    std::mutex mu;
};

static int vpcsum_group_wait_locked(vpcsum_group* g, vpcsum_group::Pending& slot) {
    int rc = 0;
    for (size_t d = 0; d < slot.sub.size(); ++d)
        if (vpcsum_ctx_wait(g->ctx[d], slot.sub[d]) != 0) rc = -1;   // every device joins, first error kept
    slot.ticket = 0;
    return rc;
}

extern "C" {

int vpcsum_group_create_list(const int* devices, int ndev, uint64_t max_arena_bytes, uint32_t max_pkts,
                             vpcsum_group_t** out) {
    try {
        if (!out || !devices || ndev <= 0 || ndev > 64) return fail("vpcsum_group_create_list: bad argument");
        std::unique_ptr<vpcsum_group> g(new vpcsum_group());
        g->ctx.reserve(ndev);   // the push_backs below cannot throw once a context exists
        for (int i = 0; i < ndev; ++i) {
            vpcsum_ctx_t* c = nullptr;
            if (vpcsum_ctx_create(devices[i], max_arena_bytes, max_pkts, &c) != 0) {
                char e[1024];
                snprintf(e, sizeof(e), "%s", g_err);
                vpcsum_group_destroy(g.release());
                return fail("%s", e);
            }
            g->ctx.push_back(c);
        }
        *out = g.release();
        return 0;
    } VPC_CATCH("vpcsum_group_create_list")
}

int vpcsum_group_create(uint64_t dev_mask, uint64_t max_arena_bytes, uint32_t max_pkts, vpcsum_group_t** out) {
    try {
        int n = 0;
        VPC_CHECK(hipGetDeviceCount(&n), "hipGetDeviceCount");
        std::vector<int> devs;
        for (int d = 0; d < 64 && d < n; ++d)
            if (dev_mask >> d & 1) devs.push_back(d);
        if (devs.empty() || (n < 64 && (dev_mask >> n) != 0))
            return fail("vpcsum_group_create: mask 0x%llx names no device or one beyond the %d present",
                        (unsigned long long)dev_mask, n);
        return vpcsum_group_create_list(devs.data(), (int)devs.size(), max_arena_bytes, max_pkts, out);
    } VPC_CATCH("vpcsum_group_create")
}

int vpcsum_group_destroy(vpcsum_group_t* g) {
    try {
        if (!g) return 0;
        int rc = 0;
        {
            // the group's batches in flight complete first (results into the callers' buffers);
            // vpcsum_ctx_destroy does the same for anything submitted to a context directly
            std::lock_guard<std::mutex> lk(g->mu);
            for (auto& slot : g->slots)
                if (slot.ticket && vpcsum_group_wait_locked(g, slot) != 0) rc = -1;
        }
        const int dev0 = g->ctx.empty() ? 0 : g->ctx[0]->device;   // the contexts are gone below
        for (auto* c : g->ctx)
            if (vpcsum_ctx_destroy(c) != 0) rc = -1;
        if (!g->reg.empty()) {
            DeviceScope on_dev(dev0);
            for (auto& r : g->reg)
                if (hostlock_release(r.key, "vpcsum_group_destroy") != 0) rc = -1;
        }
        delete g;
        return rc;
    } VPC_CATCH("vpcsum_group_destroy")
}

int vpcsum_group_register_arena(vpcsum_group_t* g, void* h_arena, uint64_t len) {
    try {
        if (!g || !h_arena || len == 0) return fail("vpcsum_group_register_arena: bad argument");
        std::lock_guard<std::mutex> lk(g->mu);
        VPC_ON_DEVICE(g->ctx[0]->device);
        // the bookkeeping may throw: make room before anything is pinned or mapped
        g->reg.reserve(g->reg.size() + 1);
        for (auto* c : g->ctx) {
            std::lock_guard<std::mutex> lc(c->mu);
            c->registered.reserve(c->registered.size() + 1);
        }
        for (auto& r : g->reg)
            if (r.host == (uint8_t*)h_arena) return fail("vpcsum_group_register_arena: %p is registered already", h_arena);
        uint8_t* key = nullptr;
        if (hostlock_acquire((uint8_t*)h_arena, len, &key, "vpcsum_group_register_arena") != 0) return -1;
        for (size_t i = 0; i < g->ctx.size(); ++i) {
            vpcsum_ctx* c = g->ctx[i];
            std::lock_guard<std::mutex> lc(c->mu);
            DeviceScope on_dev(c->device);
            void* dev = nullptr;
            hipError_t e = on_dev.err;
            if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, h_arena, 0);
            if (e != hipSuccess) {
                // roll back: no context keeps a mapping of an arena the group failed to register, so
                // a retry starts from scratch
                for (size_t q = 0; q < i; ++q) {
                    std::lock_guard<std::mutex> lq(g->ctx[q]->mu);
                    auto& rq = g->ctx[q]->registered;
                    for (size_t k = rq.size(); k-- > 0;)
                        if (rq[k].host == (uint8_t*)h_arena && !rq[k].key) rq.erase(rq.begin() + k);
                }
                (void)hostlock_release(key, "vpcsum_group_register_arena");
                return hipfail(e, "vpcsum_group_register_arena: device mapping");
            }
            c->registered.push_back({(uint8_t*)h_arena, len, (uint8_t*)dev, nullptr});
        }
        g->reg.push_back({(uint8_t*)h_arena, key});
        return 0;
    } VPC_CATCH("vpcsum_group_register_arena")
}

int vpcsum_group_unregister_arena(vpcsum_group_t* g, void* h_arena) {
    try {
        if (!g || !h_arena) return fail("vpcsum_group_unregister_arena: bad argument");
        std::lock_guard<std::mutex> lk(g->mu);
        auto it = std::find_if(g->reg.begin(), g->reg.end(),
                               [&](const vpcsum_group::Reg& r) { return r.host == (uint8_t*)h_arena; });
        if (it == g->reg.end()) return fail("vpcsum_group_unregister_arena: arena not registered");
        // Two phases, so that a failure leaves the registration whole and a retry can succeed:
        // (1) every context finishes its zero-copy batches -- the only step that can fail, and
        // nothing has been dropped yet; (2) every context forgets the mapping (the contexts do not own
        // the page-lock) and the group unpins the arena.
        for (auto* c : g->ctx) {
            std::lock_guard<std::mutex> lc(c->mu);
            DeviceScope on_dev(c->device);
            if (on_dev.err != hipSuccess) return hipfail(on_dev.err, "hipSetDevice");
            if (ctx_quiesce_zero_copy(c) != 0) return -1;
        }
        for (auto* c : g->ctx) {
            std::lock_guard<std::mutex> lc(c->mu);
            auto& r = c->registered;
            for (size_t k = r.size(); k-- > 0;)
                if (r[k].host == (uint8_t*)h_arena && !r[k].key) r.erase(r.begin() + k);
        }
        uint8_t* key = it->key;
        g->reg.erase(it);
        VPC_ON_DEVICE(g->ctx[0]->device);
        return hostlock_release(key, "vpcsum_group_unregister_arena");
    } VPC_CATCH("vpcsum_group_unregister_arena")
}

}  // extern "C"

// Byte-balanced contiguous cuts of a host batch over the group's contexts (shard_by_bytes in
// vproxy_amd/shard.py); submit(d, a, b, &ticket) hands range [a, b) to context d.  A range a
// context refuses fails the group submit only after the ranges already submitted have finished:
// they write into the caller's buffers, which the caller may free once the error is back.
template <class Submit>
static int group_submit_ranges(vpcsum_group* g, const vpcsum_desc_t* h_desc, uint32_t n, uint64_t* ticket,
                               Submit submit) {
    const uint64_t t = g->next_ticket++;
    auto& slot = g->slots[t & 1];
    if (slot.ticket && vpcsum_group_wait_locked(g, slot) != 0) return -1;
    const size_t k = g->ctx.size();
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += h_desc[i].l3_len;
    std::vector<uint32_t> cut(k + 1, n);
    cut[0] = 0;
    uint64_t acc = 0;
    size_t r = 1;
    for (uint32_t i = 0; i < n && r < k; ++i) {
        acc += h_desc[i].l3_len;
        while (r < k && acc * k >= total * r) cut[r++] = i + 1;
    }
    slot.sub.assign(k, 0);
    for (size_t d = 0; d < k; ++d) {
        const uint32_t a = cut[d], b = std::max(cut[d], cut[d + 1]);
        if (submit(d, a, b, &slot.sub[d]) != 0) {
            char e[1024];
            snprintf(e, sizeof(e), "%s", g_err);
            for (size_t q = 0; q < d; ++q) (void)vpcsum_ctx_wait(g->ctx[q], slot.sub[q]);
            slot.sub.clear();
            return fail("%s", e);
        }
    }
    slot.ticket = t;
    *ticket = t;
    return 0;
}

extern "C" {

int vpcsum_group_submit(vpcsum_group_t* g, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                        uint32_t n, uint32_t* h_out, uint8_t* h_status, uint32_t mode, uint64_t* ticket) {
    try {
        if (!g || !ticket) return fail("vpcsum_group_submit: NULL group or ticket");
        if (n && (!h_arena || !h_desc)) return fail("vpcsum_group_submit: NULL arena or descriptors");
        std::lock_guard<std::mutex> lk(g->mu);
        return group_submit_ranges(g, h_desc, n, ticket, [&](size_t d, uint32_t a, uint32_t b, uint64_t* t) {
            return vpcsum_ctx_submit(g->ctx[d], h_arena, arena_len, h_desc + a, b - a, h_out ? h_out + a : nullptr,
                                     h_status ? h_status + a : nullptr, mode, t);
        });
    } VPC_CATCH("vpcsum_group_submit")
}

int vpcsum_group_nat_submit(vpcsum_group_t* g, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                            const vpcsum_nat_t* h_rw, uint32_t n, uint8_t* h_status, uint32_t nat_mode,
                            uint64_t* ticket) {
    try {
        if (!g || !ticket) return fail("vpcsum_group_nat_submit: NULL group or ticket");
        if (n && (!h_arena || !h_desc || !h_rw)) return fail("vpcsum_group_nat_submit: NULL arena, descriptors or rewrites");
        std::lock_guard<std::mutex> lk(g->mu);
        return group_submit_ranges(g, h_desc, n, ticket, [&](size_t d, uint32_t a, uint32_t b, uint64_t* t) {
            return vpcsum_ctx_nat_submit(g->ctx[d], h_arena, arena_len, h_desc + a, h_rw + a, b - a,
                                         h_status ? h_status + a : nullptr, nat_mode, t);
        });
    } VPC_CATCH("vpcsum_group_nat_submit")
}

int vpcsum_group_submit_pre(vpcsum_group_t* g, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                            const void* h_pre, uint32_t pre_fmt, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                            uint32_t mode, uint64_t* ticket) {
    try {
        if (!g || !ticket) return fail("vpcsum_group_submit_pre: NULL group or ticket");
        if (n && (!h_arena || !h_desc || !h_pre)) return fail("vpcsum_group_submit_pre: NULL arena, descriptors or pre-images");
        if (pre_fmt > VPCSUM_PRE_FMT_PRE) return fail("vpcsum_group_submit_pre: bad pre_fmt %u", pre_fmt);
        const size_t esz = pre_fmt == VPCSUM_PRE_FMT_PRE ? sizeof(vpcsum_pre_t) : sizeof(vpcsum_pre4_t);
        std::lock_guard<std::mutex> lk(g->mu);
        return group_submit_ranges(g, h_desc, n, ticket, [&](size_t d, uint32_t a, uint32_t b, uint64_t* t) {
            return vpcsum_ctx_submit_pre(g->ctx[d], h_arena, arena_len, h_desc + a, (const uint8_t*)h_pre + a * esz, pre_fmt,
                                         b - a, h_out ? h_out + a : nullptr, h_status ? h_status + a : nullptr, mode, t);
        });
    } VPC_CATCH("vpcsum_group_submit_pre")
}

int vpcsum_group_wait(vpcsum_group_t* g, uint64_t ticket) {
    try {
        if (!g) return fail("vpcsum_group_wait: NULL group");
        std::lock_guard<std::mutex> lk(g->mu);
        auto& slot = g->slots[ticket & 1];
        if (slot.ticket != ticket) {
            if (ticket == 0 || ticket >= g->next_ticket) return fail("vpcsum_group_wait: unknown ticket %llu", (unsigned long long)ticket);
            return 0;   // already completed
        }
        return vpcsum_group_wait_locked(g, slot);
    } VPC_CATCH("vpcsum_group_wait")
}

// SURVEY.md §8(b)'s entry points over one process-wide device group (vpcsum_init creates it).
// Every call on the group holds a shared lock for its whole duration and vpcsum_init /
// vpcsum_shutdown an exclusive one: a shutdown on one thread waits for the submits and waits in
// flight on others and completes every batch still pending (vpcsum_group_destroy: results into
// the callers' buffers); a call after it fails with "vpcsum_init first" (never a freed group).
// A handle carries the generation of the group that issued it (bits 48..63; each vpcsum_init
// starts a new one), so that a handle from before a shutdown is refused by the next group instead
// of naming one of its tickets.
}  // extern "C"

static std::shared_mutex g_default_rw;
static vpcsum_group* g_default = nullptr;
static uint64_t g_default_gen = 0;   // generation of g_default (written under the exclusive lock)
constexpr int kGenShift = 48;
constexpr uint64_t kTicketMask = (1ull << kGenShift) - 1;

template <class F>
static int with_default_group(const char* what, F f) {
    std::shared_lock<std::shared_mutex> lk(g_default_rw);
    if (!g_default) return fail("%s: vpcsum_init first", what);
    return f(g_default);
}

// a submit's group ticket -> the handle the caller gets
static int default_handle(int rc, uint64_t* handle) {
    if (rc == 0 && handle) *handle = (*handle & kTicketMask) | (g_default_gen << kGenShift);
    return rc;
}

extern "C" {

int vpcsum_init(uint64_t dev_mask, uint64_t max_arena_bytes, uint32_t max_pkts) {
    try {
        std::unique_lock<std::shared_mutex> lk(g_default_rw);
        if (g_default) return fail("vpcsum_init: already initialised (vpcsum_shutdown first)");
        vpcsum_group_t* g = nullptr;
        if (vpcsum_group_create(dev_mask, max_arena_bytes, max_pkts, &g) != 0) return -1;
        g_default = g;
        g_default_gen = (g_default_gen + 1) & 0xffff ? (g_default_gen + 1) & 0xffff : 1;
        return 0;
    } VPC_CATCH("vpcsum_init")
}

int vpcsum_shutdown(void) {
    try {
        std::unique_lock<std::shared_mutex> lk(g_default_rw);
        vpcsum_group_t* g = g_default;
        g_default = nullptr;
        return vpcsum_group_destroy(g);
    } VPC_CATCH("vpcsum_shutdown")
}

int vpcsum_register_arena(void* h_arena, uint64_t len) {
    try {
        return with_default_group("vpcsum_register_arena",
                                  [&](vpcsum_group* g) { return vpcsum_group_register_arena(g, h_arena, len); });
    } VPC_CATCH("vpcsum_register_arena")
}

int vpcsum_batch_submit(uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, uint32_t n,
                        uint32_t* h_out, uint8_t* h_status, uint32_t mode, uint64_t* handle) {
    try {
        return with_default_group("vpcsum_batch_submit", [&](vpcsum_group* g) {
            return default_handle(vpcsum_group_submit(g, h_arena, arena_len, h_desc, n, h_out, h_status, mode, handle),
                                  handle);
        });
    } VPC_CATCH("vpcsum_batch_submit")
}

int vpcsum_batch_submit_pre(uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, const void* h_pre,
                            uint32_t pre_fmt, uint32_t n, uint32_t* h_out, uint8_t* h_status, uint32_t mode,
                            uint64_t* handle) {
    try {
        return with_default_group("vpcsum_batch_submit_pre", [&](vpcsum_group* g) {
            return default_handle(vpcsum_group_submit_pre(g, h_arena, arena_len, h_desc, h_pre, pre_fmt, n, h_out, h_status,
                                                          mode, handle),
                                  handle);
        });
    } VPC_CATCH("vpcsum_batch_submit_pre")
}

int vpcsum_nat_submit(uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, const vpcsum_nat_t* h_rw,
                      uint32_t n, uint8_t* h_status, uint32_t nat_mode, uint64_t* handle) {
    try {
        return with_default_group("vpcsum_nat_submit", [&](vpcsum_group* g) {
            return default_handle(vpcsum_group_nat_submit(g, h_arena, arena_len, h_desc, h_rw, n, h_status, nat_mode, handle),
                                  handle);
        });
    } VPC_CATCH("vpcsum_nat_submit")
}

int vpcsum_batch_wait(uint64_t handle) {
    try {
        return with_default_group("vpcsum_batch_wait", [&](vpcsum_group* g) {
            if ((handle >> kGenShift) != g_default_gen)
                return fail("vpcsum_batch_wait: handle 0x%llx is from before vpcsum_shutdown (its batch was completed "
                            "by the shutdown)",
                            (unsigned long long)handle);
            return vpcsum_group_wait(g, handle & kTicketMask);
        });
    } VPC_CATCH("vpcsum_batch_wait")
}

// ------------------------------------------------------------------------------------------
// PNI entry points
// ------------------------------------------------------------------------------------------
// The exception travels in env->ex as PNIThrowException stores it (pni.h:74-80); errno_ carries
// EINVAL for argument errors, ENOMEM when host memory ran out and EIO for failures of the device
// runtime (PNIStoreErrno's slot, pni.h:86-89), so Java code that inspects it sees a meaningful value.
static int pni_throw(void* env, const char* type) {
    PNIException_vpcsum* ex = (PNIException_vpcsum*)env;
    ex->type = (char*)type;
    strncpy(ex->message, g_err, sizeof(ex->message));
    ex->message[sizeof(ex->message) - 1] = '\0';
    ex->errno_ = strcmp(type, "java.lang.IllegalArgumentException") == 0 ? EINVAL
                 : strcmp(type, "java.lang.OutOfMemoryError") == 0       ? ENOMEM
                                                                         : EIO;
    return -1;
}

}  // extern "C"

// An entry point that returns a long (a ticket, a handle): `bad` arguments throw
// IllegalArgumentException with bad_msg, a failed call(&value) IOException with the library's message.
template <class Call>
static int pni_returning(PNIEnv_vpcsum_long* env, const char* name, bool bad, const char* bad_msg, Call call) {
    try {
        if (bad) {
            fail("%s", bad_msg);
            return pni_throw(env, "java.lang.IllegalArgumentException");
        }
        uint64_t value = 0;
        if (call(&value) != 0) return pni_throw(env, "java.io.IOException");
        env->return_ = (int64_t)value;
        return 0;
    } VPC_CATCH_PNI(name)
}

extern "C" {

int Java_io_vproxy_vpcsum_VPCsum_create(PNIEnv_vpcsum_long* env, int32_t device, int64_t maxArena, int32_t maxPkts) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_create", maxArena <= 0 || maxPkts <= 0,
                         "maxArena and maxPkts must be positive", [&](uint64_t* handle) {
        vpcsum_ctx_t* c = nullptr;
        const int rc = vpcsum_ctx_create(device, (uint64_t)maxArena, (uint32_t)maxPkts, &c);
        *handle = (uint64_t)(uintptr_t)c;
        return rc;
    });
}

int Java_io_vproxy_vpcsum_VPCsum_registerArena(PNIEnv_vpcsum_void* env, int64_t ctx, void* arena, int64_t len) {
    try {
        if (len <= 0) {
            fail("len must be positive");
            return pni_throw(env, "java.lang.IllegalArgumentException");
        }
        if (vpcsum_ctx_register_arena((vpcsum_ctx_t*)(intptr_t)ctx, arena, (uint64_t)len) != 0)
            return pni_throw(env, "java.io.IOException");
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_registerArena")
}

int Java_io_vproxy_vpcsum_VPCsum_submit(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                        int32_t n, void* out, void* status, int32_t mode) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_submit", n < 0 || arenaLen < 0, "negative length", [&](uint64_t* t) {
        return vpcsum_ctx_submit((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)arena, (uint64_t)arenaLen, (const vpcsum_desc_t*)desc,
                                 (uint32_t)n, (uint32_t*)out, (uint8_t*)status, (uint32_t)mode, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_waitFor(PNIEnv_vpcsum_void* env, int64_t ctx, int64_t ticket) {
    try {
        if (vpcsum_ctx_wait((vpcsum_ctx_t*)(intptr_t)ctx, (uint64_t)ticket) != 0) return pni_throw(env, "java.io.IOException");
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_waitFor")
}

int Java_io_vproxy_vpcsum_VPCsum_verifyFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                              void* frameOff, void* frameLen, int32_t n, void* out, void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_verifyFrames", n < 0 || arenaLen < 0,
                         "verifyFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_verify_frames((vpcsum_ctx_t*)(intptr_t)ctx, (const uint8_t*)arena, (uint64_t)arenaLen,
                                        (const uint64_t*)frameOff, (const uint32_t*)frameLen, (uint32_t)n, (uint32_t*)out,
                                        (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_verifyFramesHsum(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                                  void* frameOff, void* frameLen, int32_t n, void* out, void* status,
                                                  void* hsum) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_verifyFramesHsum", n < 0 || arenaLen < 0,
                         "verifyFramesHsum: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_verify_frames_hsum((vpcsum_ctx_t*)(intptr_t)ctx, (const uint8_t*)arena, (uint64_t)arenaLen,
                                             (const uint64_t*)frameOff, (const uint32_t*)frameLen, (uint32_t)n,
                                             (uint32_t*)out, (uint8_t*)status, (vpcsum_hsum_t*)hsum, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_egressFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                              void* frameOff, void* frameLen, void* frameFlags, int32_t n, void* out,
                                              void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_egressFrames", n < 0 || arenaLen < 0,
                         "egressFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_egress_frames((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)arena, (uint64_t)arenaLen,
                                        (const uint64_t*)frameOff, (const uint32_t*)frameLen, (const uint8_t*)frameFlags,
                                        (uint32_t)n, (uint32_t*)out, (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_parseFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                             void* frameOff, void* frameLen, int32_t n, void* desc, void* status,
                                             void* tuples) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_parseFrames", n < 0 || arenaLen < 0,
                         "parseFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_parse_frames((vpcsum_ctx_t*)(intptr_t)ctx, (const uint8_t*)arena, (uint64_t)arenaLen,
                                       (const uint64_t*)frameOff, (const uint32_t*)frameLen, (uint32_t)n,
                                       (vpcsum_desc_t*)desc, (uint8_t*)status, (vpcsum_tuple_t*)tuples, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_submitPre(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                           void* desc, void* pre, int32_t n, void* out, void* status, int32_t mode) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_submitPre", n < 0 || arenaLen < 0, "submitPre: negative size",
                         [&](uint64_t* t) {
        return vpcsum_ctx_submit_pre((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)arena, (uint64_t)arenaLen,
                                     (const vpcsum_desc_t*)desc, pre, VPCSUM_PRE_FMT_PRE, (uint32_t)n, (uint32_t*)out,
                                     (uint8_t*)status, (uint32_t)mode, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_natSubmit(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                           void* desc, void* rw, int32_t n, void* status, int32_t natMode) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_natSubmit", n < 0 || arenaLen < 0, "natSubmit: negative size",
                         [&](uint64_t* t) {
        return vpcsum_ctx_nat_submit((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)arena, (uint64_t)arenaLen,
                                     (const vpcsum_desc_t*)desc, (const vpcsum_nat_t*)rw, (uint32_t)n, (uint8_t*)status,
                                     (uint32_t)natMode, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_flowtabCreate(PNIEnv_vpcsum_long* env, int32_t device, int32_t maxFlows) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_flowtabCreate", maxFlows <= 0, "maxFlows must be positive",
                         [&](uint64_t* handle) {
        vpcsum_flowtab_t* f = nullptr;
        const int rc = vpcsum_flowtab_create(device, (uint32_t)maxFlows, &f);
        *handle = (uint64_t)(uintptr_t)f;
        return rc;
    });
}

int Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate(PNIEnv_vpcsum_void* env, int64_t tab, void* del, int32_t nDel, void* add,
                                               int32_t nAdd) {
    try {
        if (nDel < 0 || nAdd < 0) {
            fail("flowtabUpdate: negative count");
            return pni_throw(env, "java.lang.IllegalArgumentException");
        }
        if (vpcsum_flowtab_update((vpcsum_flowtab_t*)(intptr_t)tab, (const vpcsum_tuple_t*)del, (uint32_t)nDel,
                                  (const vpcsum_flow_t*)add, (uint32_t)nAdd, nullptr) != 0)
            return pni_throw(env, "java.io.IOException");
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate")
}

int Java_io_vproxy_vpcsum_VPCsum_flowtabCollect(PNIEnv_vpcsum_int* env, int64_t tab, void* cookies, int32_t cap) {
    try {
        if (cap < 0) {
            fail("flowtabCollect: negative capacity");
            return pni_throw(env, "java.lang.IllegalArgumentException");
        }
        uint32_t cnt = 0;
        if (vpcsum_flowtab_collect((vpcsum_flowtab_t*)(intptr_t)tab, (uint64_t*)cookies, (uint32_t)cap, &cnt, nullptr) != 0)
            return pni_throw(env, "java.io.IOException");
        env->return_ = (int32_t)cnt;
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_flowtabCollect")
}

int Java_io_vproxy_vpcsum_VPCsum_flowtabClose(PNIEnv_vpcsum_void* env, int64_t tab) {
    try {
        (void)env;
        vpcsum_flowtab_destroy((vpcsum_flowtab_t*)(intptr_t)tab);
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_flowtabClose")
}

int Java_io_vproxy_vpcsum_VPCsum_natFlowFrames(PNIEnv_vpcsum_long* env, int64_t ctx, int64_t tab, void* arena,
                                               int64_t arenaLen, void* frameOff, void* frameLen, int32_t n, void* status,
                                               void* verdict, int32_t natMode) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_natFlowFrames", n < 0 || arenaLen < 0,
                         "natFlowFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_nat_flow_frames((vpcsum_ctx_t*)(intptr_t)ctx, (vpcsum_flowtab_t*)(intptr_t)tab, (uint8_t*)arena,
                                          (uint64_t)arenaLen, (const uint64_t*)frameOff, (const uint32_t*)frameLen,
                                          (uint32_t)n, (uint8_t*)status, (uint8_t*)verdict, (uint32_t)natMode, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(PNIEnv_vpcsum_int* env, int64_t tab, void* keys, void* fp, int32_t n) {
    try {
        if (n < 0) {
            fail("flowtabSetFastpath: negative count");
            return pni_throw(env, "java.lang.IllegalArgumentException");
        }
        uint32_t missing = 0;
        if (vpcsum_flowtab_set_fastpath((vpcsum_flowtab_t*)(intptr_t)tab, (const vpcsum_tuple_t*)keys,
                                        (const vpcsum_fastpath_t*)fp, (uint32_t)n, &missing, nullptr) != 0)
            return pni_throw(env, "java.io.IOException");
        env->return_ = (int32_t)missing;
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath")
}

int Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames(PNIEnv_vpcsum_long* env, int64_t ctx, int64_t tab, void* arena,
                                                      int64_t arenaLen, void* frameOff, void* frameLen, int32_t n,
                                                      void* status, void* verdict, void* port, int32_t natMode) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames", n < 0 || arenaLen < 0,
                         "natFlowForwardFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_nat_flow_forward_frames((vpcsum_ctx_t*)(intptr_t)ctx, (vpcsum_flowtab_t*)(intptr_t)tab,
                                                  (uint8_t*)arena, (uint64_t)arenaLen, (const uint64_t*)frameOff,
                                                  (const uint32_t*)frameLen, (uint32_t)n, (uint8_t*)status, (uint8_t*)verdict,
                                                  (uint32_t*)port, (uint32_t)natMode, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* dst, int64_t dstLen, void* src,
                                                int64_t srcLen, void* hdr, int32_t nHdr, void* seg, int32_t n,
                                                void* frameLen, void* out, void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames", n < 0 || nHdr < 0 || dstLen < 0 || srcLen < 0,
                         "buildTcpFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_build_tcp_frames((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)dst, (uint64_t)dstLen, (const uint8_t*)src,
                                           (uint64_t)srcLen, (const vpcsum_tcphdr_t*)hdr, (uint32_t)nHdr,
                                           (const vpcsum_tcpseg_t*)seg, (uint32_t)n, (uint32_t*)frameLen, (uint32_t*)out,
                                           (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts(PNIEnv_vpcsum_long* env, int64_t ctx, void* dst, int64_t dstLen, void* src,
                                                int64_t srcLen, void* hdr, int32_t nHdr, void* burst, int32_t nBursts,
                                                void* frameOff, int32_t nFrames, int32_t frameCap, void* frameLen,
                                                void* out, void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts",
                         nFrames < 0 || nBursts < 0 || nHdr < 0 || frameCap < 0 || dstLen < 0 || srcLen < 0,
                         "buildTcpBursts: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_build_tcp_bursts((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)dst, (uint64_t)dstLen, (const uint8_t*)src,
                                           (uint64_t)srcLen, (const vpcsum_tcphdr_t*)hdr, (uint32_t)nHdr,
                                           (const vpcsum_tcpburst_t*)burst, (uint32_t)nBursts, (const uint64_t*)frameOff,
                                           (uint32_t)nFrames, (uint32_t)frameCap, (uint32_t*)frameLen, (uint32_t*)out,
                                           (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                               void* rx, int32_t n, void* dst, int64_t dstLen, void* stored, void* out,
                                               void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames", n < 0 || arenaLen < 0 || dstLen < 0,
                         "recvTcpFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_recv_tcp_frames((vpcsum_ctx_t*)(intptr_t)ctx, (const uint8_t*)arena, (uint64_t)arenaLen,
                                          (const vpcsum_desc_t*)desc, (const vpcsum_tcprx_t*)rx, (uint32_t)n, (uint8_t*)dst,
                                          (uint64_t)dstLen, (uint32_t*)stored, (uint32_t*)out, (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* dst, int64_t dstLen, void* src,
                                                int64_t srcLen, void* hdr, int32_t nHdr, void* dg, int32_t n,
                                                void* frameLen, void* out, void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames", n < 0 || nHdr < 0 || dstLen < 0 || srcLen < 0,
                         "buildUdpFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_build_udp_frames((vpcsum_ctx_t*)(intptr_t)ctx, (uint8_t*)dst, (uint64_t)dstLen, (const uint8_t*)src,
                                           (uint64_t)srcLen, (const vpcsum_udphdr_t*)hdr, (uint32_t)nHdr,
                                           (const vpcsum_udpdg_t*)dg, (uint32_t)n, (uint32_t*)frameLen, (uint32_t*)out,
                                           (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                               void* rx, int32_t n, void* dst, int64_t dstLen, void* stored, void* out,
                                               void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames", n < 0 || arenaLen < 0 || dstLen < 0,
                         "recvUdpFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_recv_udp_frames((vpcsum_ctx_t*)(intptr_t)ctx, (const uint8_t*)arena, (uint64_t)arenaLen,
                                          (const vpcsum_desc_t*)desc, (const vpcsum_udprx_t*)rx, (uint32_t)n, (uint8_t*)dst,
                                          (uint64_t)dstLen, (uint32_t*)stored, (uint32_t*)out, (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                                 void* hdr, int32_t nHdr, void* rp, int32_t n, void* dst, int64_t dstLen,
                                                 void* frameLen, void* csum, void* out, void* status) {
    return pni_returning(env, "Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames", n < 0 || nHdr < 0 || arenaLen < 0 || dstLen < 0,
                         "replyIcmpFrames: negative size", [&](uint64_t* t) {
        return vpcsum_ctx_reply_icmp_frames((vpcsum_ctx_t*)(intptr_t)ctx, (const uint8_t*)arena, (uint64_t)arenaLen,
                                            (const vpcsum_desc_t*)desc, (const vpcsum_icmphdr_t*)hdr, (uint32_t)nHdr,
                                            (const vpcsum_icmprp_t*)rp, (uint32_t)n, (uint8_t*)dst, (uint64_t)dstLen,
                                            (uint32_t*)frameLen, (uint32_t*)csum, (uint32_t*)out, (uint8_t*)status, t);
    });
}

int Java_io_vproxy_vpcsum_VPCsum_setService(PNIEnv_vpcsum_void* env, int64_t ctx, int32_t idleUs) {
    try {
        if (idleUs < 0) {
            fail("setService: negative idle time %d", idleUs);
            return pni_throw(env, "java.lang.IllegalArgumentException");
        }
        if (vpcsum_ctx_set_service((vpcsum_ctx_t*)(intptr_t)ctx, (uint32_t)idleUs) != 0) return pni_throw(env, "java.io.IOException");
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_setService")
}

int Java_io_vproxy_vpcsum_VPCsum_close(PNIEnv_vpcsum_void* env, int64_t ctx) {
    try {
        (void)env;
        vpcsum_ctx_destroy((vpcsum_ctx_t*)(intptr_t)ctx);
        return 0;
    } VPC_CATCH_PNI("Java_io_vproxy_vpcsum_VPCsum_close")
}

}  // extern "C"
