// The flow table's Fastpath records (vproxy_amd/csrc/flow_table.h: FlowSlot::fp, set_fastpath) against
// a std::map model, stand-alone under ASan / UBSan (tests/test_fastpath_cpu.py builds and runs it;
// nothing of the library is linked): random insert / replace / erase / set_fastpath steps on the
// smallest table (8 slots) and on a 1,024-slot one.  After every step each live key's record equals
// the model's: kept by a replace, moved with its flow by an erase's backward shift, gone after erase
// and re-insert, all zeros after port 0; empty slots are all zeros.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "flow_table.h"

using namespace vpcsum;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_rng = 0x13198a2e03707344ull;
static uint64_t rnd() {
    g_rng += 0x9e3779b97f4a7c15ull;
    return flow_mix(g_rng);
}

struct Model {
    uint64_t cookie;
    vpcsum_fastpath_t fp;   // all zeros: none
};

static std::string key_of(const vpcsum_tuple_t& k) { return std::string((const char*)&k, kFlowKeyBytes); }

static vpcsum_tuple_t make_key(uint32_t i) {
    vpcsum_tuple_t k;
    memset(&k, 0, sizeof(k));
    const bool v6 = i & 1;
    const uint64_t a = flow_mix(i * 2 + 1), b = flow_mix(i * 2 + 2);
    memcpy(k.src, &a, v6 ? 8 : 4);
    memcpy(k.dst, &b, v6 ? 8 : 4);
    if (v6) { memcpy(k.src + 8, &b, 8); memcpy(k.dst + 8, &a, 8); }
    k.sport[0] = (uint8_t)(i >> 8); k.sport[1] = (uint8_t)i;
    k.l3_ver = v6 ? 6 : 4;
    k.l4_proto = (i & 2) ? 6 : 17;
    return k;
}

static vpcsum_flow_t make_flow(const vpcsum_tuple_t& k) {
    vpcsum_flow_t f;
    memset(&f, 0, sizeof(f));
    f.key = k;
    for (size_t j = 0; j < 36; ++j) ((uint8_t*)&f.rw)[j] = (uint8_t)rnd();
    f.cookie = rnd();
    return f;
}

// a record with every byte random; port 0 one time in four
static vpcsum_fastpath_t make_fp() {
    vpcsum_fastpath_t p;
    for (size_t j = 0; j < 12; ++j) ((uint8_t*)&p)[j] = (uint8_t)rnd();
    p.port = rnd() % 4 == 0 ? 0u : (uint32_t)rnd() | 1u;
    return p;
}

static void check_table(const FlowTable& t, const std::map<std::string, Model>& model) {
    static const FlowSlot zero = {};
    CHECK(t.flows() == model.size(), "%u flows, model %zu", t.flows(), model.size());
    const FlowSlot* s = t.data();
    uint32_t occupied = 0;
    for (uint32_t i = 0; i < t.slots(); ++i) {
        if (!s[i].occupied) {
            CHECK(memcmp(&s[i], &zero, sizeof(FlowSlot)) == 0, "empty slot %u is not all zeros", i);
            continue;
        }
        ++occupied;
        const auto it = model.find(key_of(s[i].key));
        CHECK(it != model.end(), "slot %u holds a key the model does not", i);
        CHECK(s[i].cookie == it->second.cookie, "slot %u: cookie", i);
        CHECK(memcmp(&s[i].fp, &it->second.fp, sizeof(vpcsum_fastpath_t)) == 0, "slot %u: Fastpath port %u, model %u", i, s[i].fp.port,
              it->second.fp.port);
        CHECK(memcmp(s[i].pad, zero.pad, sizeof(zero.pad)) == 0, "slot %u: padding written", i);
    }
    CHECK(occupied == model.size(), "%u occupied slots", occupied);
}

static void refusals(FlowTable& t, const std::map<std::string, Model>& model) {
    vpcsum_tuple_t good = make_key(4);   // IPv4
    std::vector<vpcsum_tuple_t> bad;
    vpcsum_tuple_t g = good; g.l4_proto = 1; bad.push_back(g);
    g = good; g.l3_ver = 5; bad.push_back(g);
    g = good; g.src[7] = 1; bad.push_back(g);
    g = good; g.dst[15] = 1; bad.push_back(g);
    g = good; g.tcp_flags = 0x10; bad.push_back(g);
    g = good; g.rsv = 1; bad.push_back(g);
    vpcsum_fastpath_t fp = make_fp();
    fp.port = 7;
    for (const auto& b : bad) {
        const char* why = nullptr;
        FlowDirty dirty(8);
        CHECK(t.set_fastpath(b, fp, &dirty, &why) == -1 && why && *why && dirty.empty(), "a malformed key was accepted");
        check_table(t, model);
    }
}

static void run(uint32_t max_flows, uint32_t want_slots, uint32_t nkeys, int steps) {
    FlowSlot* mem = (FlowSlot*)aligned_alloc(128, (size_t)want_slots * sizeof(FlowSlot));
    CHECK(mem, "aligned_alloc");
    memset((void*)mem, 0, (size_t)want_slots * sizeof(FlowSlot));
    {
        FlowTable t(max_flows, mem);
        CHECK(t.slots() == want_slots, "slots");
        std::vector<vpcsum_tuple_t> universe;
        for (uint32_t i = 0; i < nkeys; ++i) universe.push_back(make_key(i));
        std::map<std::string, Model> model;
        uint32_t kept = 0, moved = 0, reborn = 0, cleared = 0, missing = 0, set = 0;
        std::map<std::string, bool> had_fp;   // keys erased while they had a Fastpath
        for (int step = 0; step < steps; ++step) {
            const vpcsum_tuple_t& k = universe[rnd() % nkeys];
            const bool filling = (step / (int)(4 * max_flows)) % 2 == 0;
            const uint32_t op = rnd() % 10;
            FlowDirty dirty(t.slots());
            const auto it = model.find(key_of(k));
            if (op < (filling ? 4u : 1u)) {
                const vpcsum_flow_t f = make_flow(k);
                const int64_t id = t.insert(f, &dirty);
                if (it != model.end()) {   // replace: the Fastpath stays
                    CHECK(id >= 0, "replace failed");
                    it->second.cookie = f.cookie;
                    if (it->second.fp.port) ++kept;
                } else if (model.size() < max_flows) {   // new: none, whatever the slot or the key held before
                    CHECK(id >= 0, "insert failed");
                    Model m;
                    m.cookie = f.cookie;
                    memset(&m.fp, 0, sizeof(m.fp));
                    model[key_of(k)] = m;
                    if (had_fp.count(key_of(k))) ++reborn;
                } else {
                    CHECK(id == -1 && dirty.empty(), "a full table took a flow");
                }
            } else if (op < (filling ? 5u : 4u)) {
                // slots holding a Fastpath before the erase, to see the backward shift move one
                std::vector<std::pair<vpcsum_tuple_t, uint32_t>> where;
                for (uint32_t i = 0; i < t.slots(); ++i)
                    if (t.data()[i].occupied && t.data()[i].fp.port) where.emplace_back(t.data()[i].key, i);
                const int64_t id = t.erase(k, &dirty);
                CHECK((id >= 0) == (it != model.end()), "erase disagrees with the model");
                if (it != model.end()) {
                    if (it->second.fp.port) had_fp[key_of(k)] = true;
                    model.erase(it);
                    for (const auto& w : where)
                        if (!flow_key_equal(w.first, k) && t.find(w.first) != (int64_t)w.second) ++moved;
                }
            } else {
                const vpcsum_fastpath_t fp = make_fp();
                const char* why = nullptr;
                const int rc = t.set_fastpath(k, fp, &dirty, &why);
                if (it == model.end()) {
                    CHECK(rc == 0 && dirty.empty() && !why, "a missing key: rc %d", rc);
                    ++missing;
                } else {
                    CHECK(rc == 1 && dirty.idx.size() == 1 && !dirty.all, "set_fastpath: rc %d", rc);
                    CHECK(dirty.idx[0] == (uint32_t)t.find(k), "set_fastpath noted another slot");
                    if (fp.port) { it->second.fp = fp; ++set; }
                    else { if (it->second.fp.port) ++cleared; memset(&it->second.fp, 0, sizeof(fp)); }   // port 0: all zeros
                }
            }
            check_table(t, model);
        }
        CHECK(kept > 0 && moved > 0 && reborn > 0 && cleared > 0 && missing > 0 && set > 0,
              "coverage: kept %u moved %u reborn %u cleared %u missing %u set %u", kept, moved, reborn, cleared, missing, set);
        refusals(t, model);
        printf("table %u slots: %d steps, %u kept by replace, %u moved by shift, %u re-inserted bare, %u cleared, %u missing\n",
               want_slots, steps, kept, moved, reborn, cleared, missing);
    }
    free(mem);
}

int main() {
    static_assert(sizeof(vpcsum_fastpath_t) == 16 && alignof(vpcsum_fastpath_t) == 4, "vpcsum_fastpath_t layout");
    static_assert(offsetof(vpcsum_fastpath_t, src) == 6 && offsetof(vpcsum_fastpath_t, port) == 12, "vpcsum_fastpath_t layout");
    static_assert(offsetof(FlowSlot, fp) == 112 && sizeof(FlowSlot) == 128, "FlowSlot layout");
    static_assert(offsetof(FlowSlot, cookie) == 96 && offsetof(FlowSlot, pad) == 104, "FlowSlot layout");
    run(4, 8, 12, 4000);
    run(512, 1024, 1400, 8000);
    printf("offsetof(FlowSlot, fp) = %zu\n", offsetof(FlowSlot, fp));
    printf("flow_fastpath ok\n");
    return 0;
}
