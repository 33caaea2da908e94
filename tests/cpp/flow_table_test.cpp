// The NAT flow table's host logic (vproxy_amd/csrc/flow_table.h) against a std::map model, stand-alone
// under ASan / UBSan (tests/test_flow_cpu.py builds and runs it; nothing of the library is linked):
// a few thousand random insert / replace / erase / lookup steps on the smallest table (8 slots) and
// on a 1,024-slot one, with the table's invariants checked after every step.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "flow_table.h"

using namespace vpcsum;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd() {
    g_rng += 0x9e3779b97f4a7c15ull;
    return flow_mix(g_rng);
}

struct Model {
    vpcsum_nat_t rw;
    uint64_t cookie;
    uint32_t id;
};

static std::string key_of(const vpcsum_tuple_t& k) { return std::string((const char*)&k, kFlowKeyBytes); }

// key number i of a small universe: IPv4 and IPv6, TCP and UDP
static vpcsum_tuple_t make_key(uint32_t i) {
    vpcsum_tuple_t k;
    memset(&k, 0, sizeof(k));
    const bool v6 = i & 1;
    const uint64_t a = flow_mix(i * 2 + 1), b = flow_mix(i * 2 + 2);
    memcpy(k.src, &a, v6 ? 8 : 4);
    memcpy(k.dst, &b, v6 ? 8 : 4);
    if (v6) { memcpy(k.src + 8, &b, 8); memcpy(k.dst + 8, &a, 8); }
    k.sport[0] = (uint8_t)(i >> 8); k.sport[1] = (uint8_t)i;
    k.dport[0] = (uint8_t)(a >> 40); k.dport[1] = (uint8_t)(a >> 48);
    k.l3_ver = v6 ? 6 : 4;
    k.l4_proto = (i & 2) ? 6 : 17;
    return k;
}

static vpcsum_flow_t make_flow(const vpcsum_tuple_t& k) {
    vpcsum_flow_t f;
    memset(&f, 0, sizeof(f));
    f.key = k;
    for (size_t j = 0; j < 36; ++j) ((uint8_t*)&f.rw)[j] = (uint8_t)rnd();
    f.rw.mask = (uint8_t)(rnd() & 0x3f);
    f.cookie = rnd();
    return f;
}

// every invariant of the table against the model
static void check_table(const FlowTable& t, const std::map<std::string, Model>& model, const std::vector<vpcsum_tuple_t>& universe) {
    CHECK(t.flows() == model.size(), "%u flows, model %zu", t.flows(), model.size());
    const FlowSlot* s = t.data();
    uint32_t occupied = 0, worst = 0;
    std::set<uint32_t> ids;
    for (uint32_t i = 0; i < t.slots(); ++i) {
        if (!s[i].occupied) {
            static const FlowSlot zero = {};
            CHECK(memcmp(&s[i], &zero, sizeof(FlowSlot)) == 0, "empty slot %u is not all zeros", i);
            continue;
        }
        ++occupied;
        CHECK(s[i].key.tcp_flags == 0 && s[i].key.rsv == 0, "slot %u: flags in the key", i);
        const auto it = model.find(key_of(s[i].key));
        CHECK(it != model.end(), "slot %u holds a key the model does not", i);
        CHECK(memcmp(&s[i].rw, &it->second.rw, sizeof(vpcsum_nat_t)) == 0 && s[i].cookie == it->second.cookie, "slot %u: entry", i);
        CHECK(s[i].flow_id == it->second.id, "slot %u: id %u, model %u", i, s[i].flow_id, it->second.id);
        CHECK(s[i].flow_id < t.max_flows() && t.live(s[i].flow_id) && t.cookie(s[i].flow_id) == s[i].cookie, "slot %u: id bookkeeping", i);
        CHECK(ids.insert(s[i].flow_id).second, "flow id %u twice", s[i].flow_id);
        // no probe chain crosses an empty slot: every slot from home to here is occupied
        const uint32_t home = (uint32_t)flow_hash(s[i].key) & t.mask();
        const uint32_t d = (i - home) & t.mask();
        for (uint32_t p = 0; p < d; ++p) CHECK(s[(home + p) & t.mask()].occupied, "slot %u: empty slot %u steps after its home", i, p);
        if (d > worst) worst = d;
    }
    CHECK(occupied == model.size(), "%u occupied slots", occupied);
    CHECK(t.max_probe() == worst, "max_probe %u, largest displacement %u", t.max_probe(), worst);
    // every key of the universe: found (within max_probe + 1 slots: find() probes no further) iff in the model
    for (const auto& k : universe) {
        const int64_t at = t.find(k);
        CHECK((at >= 0) == (model.count(key_of(k)) != 0), "find disagrees with the model");
        if (at >= 0) CHECK(flow_key_equal(s[at].key, k), "find returned another key's slot");
    }
}

static void refusals(FlowTable& t, const std::map<std::string, Model>& model, const std::vector<vpcsum_tuple_t>& universe) {
    std::vector<vpcsum_flow_t> bad;
    vpcsum_flow_t f = make_flow(make_key(4));   // IPv4
    CHECK(f.key.l3_ver == 4, "key 4 is IPv4");
    vpcsum_flow_t g = f; g.key.l4_proto = 1; bad.push_back(g);
    g = f; g.key.l4_proto = 58; bad.push_back(g);
    g = f; g.key.l3_ver = 0; bad.push_back(g);
    g = f; g.key.l3_ver = 5; bad.push_back(g);
    for (int b = 4; b < 16; ++b) {
        g = f; g.key.src[b] = 1; bad.push_back(g);
        g = f; g.key.dst[b] = 0x80; bad.push_back(g);
    }
    g = f; g.key.tcp_flags = 0x10; bad.push_back(g);
    g = f; g.key.rsv = 1; bad.push_back(g);
    for (const auto& b : bad) {
        const char* why = nullptr;
        FlowDirty dirty(8);
        CHECK(t.insert(b, &dirty, &why) == -1 && why && *why && dirty.empty(), "a malformed key was inserted");
        std::string msg;
        const vpcsum_flow_t two[2] = {make_flow(make_key(6)), b};
        CHECK(!t.validate(nullptr, 0, two, 2, &msg) && !msg.empty(), "validate accepts a malformed key");
        check_table(t, model, universe);
    }
    // an IPv6 key may use all 16 address bytes
    CHECK(flow_key_refusal(make_key(5)) == nullptr && make_key(5).src[12] != 0, "IPv6 key");
}

static void run(uint32_t max_flows, uint32_t want_slots, uint32_t nkeys, int steps) {
    CHECK(FlowTable::slots_for(max_flows) == want_slots, "slots_for(%u) = %u", max_flows, FlowTable::slots_for(max_flows));
    // exact size: a slot past the end is the sanitizer's to report
    FlowSlot* mem = (FlowSlot*)aligned_alloc(128, (size_t)want_slots * sizeof(FlowSlot));
    CHECK(mem, "aligned_alloc");
    memset((void*)mem, 0, (size_t)want_slots * sizeof(FlowSlot));
    {
        FlowTable t(max_flows, mem);
        CHECK(t.slots() == want_slots && t.slots() >= 2 * max_flows && (t.slots() & (t.slots() - 1)) == 0, "slots");
        std::vector<vpcsum_tuple_t> universe;
        for (uint32_t i = 0; i < nkeys; ++i) universe.push_back(make_key(i));
        std::map<std::string, Model> model;
        std::set<uint32_t> free_ids;
        check_table(t, model, universe);
        uint32_t full_refusals = 0, replaces = 0, erases = 0, wraps = 0;
        for (int step = 0; step < steps; ++step) {
            const vpcsum_tuple_t& k = universe[rnd() % nkeys];
            // phases that fill the table to its limit and drain it again
            const bool filling = (step / (int)(4 * max_flows)) % 2 == 0;
            const uint32_t op = rnd() % 8;
            FlowDirty dirty(t.slots());
            if (op < (filling ? 6u : 2u)) {
                vpcsum_flow_t f = make_flow(k);
                f.key.tcp_flags = 0;
                const auto it = model.find(key_of(k));
                const char* why = nullptr;
                std::string vmsg;
                const bool vok = t.validate(nullptr, 0, &f, 1, &vmsg);
                const int64_t id = t.insert(f, &dirty, &why);
                if (it != model.end()) {   // replace: the id stays
                    CHECK(id == (int64_t)it->second.id && vok, "replace changed the id");
                    it->second.rw = f.rw;
                    it->second.cookie = f.cookie;
                    ++replaces;
                } else if (model.size() >= max_flows) {   // full: refused, nothing changed
                    CHECK(id == -1 && why && dirty.empty() && !vok && vmsg.find("full") != std::string::npos, "a full table took a flow");
                    ++full_refusals;
                } else {
                    CHECK(id >= 0 && id < (int64_t)max_flows && vok, "insert failed: %s", why ? why : "?");
                    for (const auto& kv : model) CHECK(kv.second.id != (uint32_t)id, "id %lld given twice", (long long)id);
                    model[key_of(k)] = Model{f.rw, f.cookie, (uint32_t)id};
                    CHECK(!dirty.empty(), "insert dirtied no slot");
                }
            } else if (op < 7) {
                const auto it = model.find(key_of(k));
                const int64_t id = t.erase(k, &dirty);
                if (it == model.end()) {
                    CHECK(id == -1 && dirty.empty(), "erased a key that was not there");
                } else {
                    CHECK(id == (int64_t)it->second.id && !t.live((uint32_t)id), "erase returned id %lld", (long long)id);
                    model.erase(it);
                    ++erases;
                }
            } else {
                // an update's validation: erase k, add two flows; equals what applying it would do
                vpcsum_flow_t add[2] = {make_flow(universe[rnd() % nkeys]), make_flow(universe[rnd() % nkeys])};
                std::set<std::string> after;
                for (const auto& kv : model) after.insert(kv.first);
                after.erase(key_of(k));
                after.insert(key_of(add[0].key));
                after.insert(key_of(add[1].key));
                CHECK(t.validate(&k, 1, add, 2, nullptr) == (after.size() <= max_flows), "validate miscounts");
            }
            CHECK(!dirty.all, "the dirty log overflowed its room");
            for (uint32_t d : dirty.idx) CHECK(d < t.slots(), "dirty slot %u", d);
            for (uint32_t i = 0; i < t.slots(); ++i) {
                if (!t.data()[i].occupied) continue;
                const uint32_t home = (uint32_t)flow_hash(t.data()[i].key) & t.mask();
                if (home > i) ++wraps;   // a chain wrapped past the last slot
            }
            check_table(t, model, universe);
        }
        // (in the 8-slot table chains wrap past slot 7 all the time; the large one need not see it)
        CHECK(full_refusals > 0 && replaces > 0 && erases > 0 && (wraps > 0 || want_slots > 8), "coverage: full %u replace %u erase %u wraps %u",
              full_refusals, replaces, erases, wraps);
        refusals(t, model, universe);
        printf("table %u slots: %d steps, %u refused full, %u replaced, %u erased\n", want_slots, steps, full_refusals, replaces, erases);
    }
    free(mem);
}

int main() {
    static_assert(sizeof(vpcsum_flow_t) == 96 && sizeof(FlowSlot) == 128 && alignof(FlowSlot) == 128, "layouts");
    static_assert(sizeof(vpcsum_tuple_t) == 40 && sizeof(vpcsum_nat_t) == 48, "layouts");
    static_assert(offsetof(vpcsum_flow_t, rw) == 40 && offsetof(vpcsum_flow_t, cookie) == 88, "vpcsum_flow_t layout");
    // the hash reads the 38 key bytes and nothing else
    vpcsum_tuple_t k = make_key(3);
    const uint64_t h = flow_hash(k);
    k.tcp_flags = 0x3f; k.rsv = 0xff;
    CHECK(flow_hash(k) == h, "the hash reads tcp_flags / rsv");
    for (int b = 0; b < kFlowKeyBytes; ++b) {
        vpcsum_tuple_t m = make_key(3);
        ((uint8_t*)&m)[b] ^= 1;
        CHECK(flow_hash(m) != h, "key byte %d is not hashed", b);
    }
    // the dirty log never grows past its room: it says "all" instead
    FlowDirty log(2);
    log.note(3); log.note(4);
    CHECK(!log.all && log.idx.size() == 2, "a log within its room");
    log.note(5);
    CHECK(log.all && log.idx.size() == 2, "a log past its room");
    run(4, 8, 12, 3000);
    run(512, 1024, 1400, 6000);
    printf("flow_table ok\n");
    return 0;
}
