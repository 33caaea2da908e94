// flow_table.h -- the NAT flow table's host logic and the layout and hash it shares with the lookup
// kernel (flow.hip): plain C++, no HIP call, testable stand-alone (tests/cpp/flow_table_test.cpp).
//
// An exact-match table from the tuple the parse writes (vpcsum_tuple_t: what TcpInput / UdpInput
// hand to conntrack.lookupTcp / lookupUdp, Conntrack.java:106-125) to the vpcsum_nat_t that
// SwitchUtils.applyNat writes for that flow direction (SwitchUtils.java:522-542).  Open addressing,
// linear probing, deletion by backward shift: there are no tombstones, so an empty slot always ends
// a probe, and no live entry lies further from its home slot than max_probe().
#pragma once
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "vpcsum.h"

#if defined(__HIPCC__)
#define VPC_FLOW_HD __host__ __device__ inline
#else
#define VPC_FLOW_HD inline
#endif

namespace vpcsum {

// One slot: 128 B, 128-B aligned, so a probe reads one cache line.  The lookup kernel's team of 8
// lanes takes 16 B each: lanes 0..2 the key (with the flow id and the occupied word), 3..5 the entry,
// lane 7 the flow's Fastpath (port 0: none).
struct alignas(128) FlowSlot {
    vpcsum_tuple_t key;   //   0: tcp_flags and rsv are 0
    uint32_t flow_id;     //  40: dense, stable for the flow's life, recycled after erase
    uint32_t occupied;    //  44: 0 = empty
    vpcsum_nat_t rw;      //  48
    uint64_t cookie;      //  96
    uint8_t pad[8];       // 104
    vpcsum_fastpath_t fp; // 112: the flow's Ethernet addresses and output port, all zeros = none
};
static_assert(sizeof(FlowSlot) == 128 && alignof(FlowSlot) == 128, "one slot is one 128-B line");
static_assert(offsetof(FlowSlot, flow_id) == 40 && offsetof(FlowSlot, occupied) == 44 && offsetof(FlowSlot, rw) == 48 &&
                  offsetof(FlowSlot, cookie) == 96,
              "FlowSlot layout (flow.hip reads it in 16-B pieces)");
static_assert(offsetof(FlowSlot, fp) == 112 && sizeof(vpcsum_fastpath_t) == 16,
              "the Fastpath is the slot's last 16-B piece (flow.hip: lane 7 holds it whole)");
static_assert(sizeof(vpcsum_flow_t) == 96, "vpcsum_flow_t is 96 bytes");

constexpr int kFlowKeyBytes = 38;   // src[16] dst[16] sport dport l3_ver l4_proto

// The hash of a key, from its five little-endian 64-bit words (the fifth without tcp_flags / rsv):
// each word mixed with a constant of its position (the splitmix64 finaliser), the five added -- so
// that the kernel's lanes can each mix the words they hold and add across the team --, the sum mixed
// once more.  slot = hash & (slots - 1).
VPC_FLOW_HD uint64_t flow_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
VPC_FLOW_HD uint64_t flow_word_hash(uint64_t w, int k) { return flow_mix(w + 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1)); }
VPC_FLOW_HD uint64_t flow_hash_words(const uint64_t w[5]) {
    uint64_t h = 0;
    for (int k = 0; k < 4; ++k) h += flow_word_hash(w[k], k);
    h += flow_word_hash(w[4] & 0x0000ffffffffffffull, 4);
    return flow_mix(h);
}

inline uint64_t flow_hash(const vpcsum_tuple_t& key) {
    uint64_t w[5];
    memcpy(w, &key, sizeof(w));   // the library's hosts and the device are little-endian
    return flow_hash_words(w);
}

inline bool flow_key_equal(const vpcsum_tuple_t& a, const vpcsum_tuple_t& b) { return memcmp(&a, &b, kFlowKeyBytes) == 0; }

// Why a key cannot be inserted, or nullptr.
inline const char* flow_key_refusal(const vpcsum_tuple_t& k) {
    if (k.l4_proto != 6 && k.l4_proto != 17) return "l4_proto is neither TCP (6) nor UDP (17)";
    if (k.l3_ver != 4 && k.l3_ver != 6) return "l3_ver is neither 4 nor 6";
    if (k.tcp_flags != 0 || k.rsv != 0) return "tcp_flags / rsv of a key must be 0";
    if (k.l3_ver == 4)
        for (int i = 4; i < 16; ++i)
            if (k.src[i] != 0 || k.dst[i] != 0) return "an IPv4 key has non-zero address bytes 4..15 (the parse writes zeros)";
    return nullptr;
}

// The slots an update wrote, for the copy to the device.  Room is made before the table changes
// and never grows: past it `all` says "copy the whole table", so that noting a slot cannot throw
// between two writes of a backward shift.
struct FlowDirty {
    std::vector<uint32_t> idx;
    size_t room;
    bool all = false;
    explicit FlowDirty(size_t room_) : room(room_) { idx.reserve(room); }
    void note(uint32_t i) {
        if (idx.size() < room) idx.push_back(i);
        else all = true;
    }
    bool empty() const { return idx.empty() && !all; }
};

// insert() and erase() allocate nothing: ids, cookies and the displacement counts have their room
// from the constructor on, so a table is never left half changed.
class FlowTable {
public:
    // max_flows >= 1; storage: `slots()` FlowSlot, zeroed, 128-B aligned, owned by the caller (the
    // library hands pinned memory; the test a vector)
    static uint32_t slots_for(uint32_t max_flows) {
        uint64_t s = 8;
        while (s < 2ull * max_flows) s <<= 1;
        return (uint32_t)s;
    }
    FlowTable(uint32_t max_flows, FlowSlot* storage)
        : slot_(storage), slots_(slots_for(max_flows)), mask_(slots_ - 1), max_flows_(max_flows), next_id_(0), flows_(0) {
        cookie_.assign(max_flows, 0);
        live_.assign(max_flows, 0);
        free_ids_.reserve(max_flows);
        disp_.assign(slots_, 0);
    }

    uint32_t slots() const { return slots_; }
    uint32_t mask() const { return mask_; }
    uint32_t flows() const { return flows_; }
    uint32_t max_flows() const { return max_flows_; }
    // the largest displacement of a live entry from its home slot (0 for an empty table)
    uint32_t max_probe() const { return max_probe_; }
    const FlowSlot* data() const { return slot_; }
    bool live(uint32_t id) const { return id < max_flows_ && live_[id] != 0; }
    uint64_t cookie(uint32_t id) const { return cookie_[id]; }

    // slot index of the key, or -1: at most max_probe() + 1 slots, ended by an empty one
    int64_t find(const vpcsum_tuple_t& key) const {
        uint32_t i = (uint32_t)flow_hash(key) & mask_;
        for (uint32_t p = 0, e = max_probe(); p <= e; ++p, i = (i + 1) & mask_) {
            if (!slot_[i].occupied) return -1;
            if (flow_key_equal(slot_[i].key, key)) return i;
        }
        return -1;
    }

    // Whether erasing del[0..n_del) and then inserting add[0..n_add) would succeed, with nothing
    // changed: a malformed key or a table that would hold more than max_flows refuses the whole
    // update (*why says which).
    bool validate(const vpcsum_tuple_t* del, uint32_t n_del, const vpcsum_flow_t* add, uint32_t n_add, std::string* why) const {
        for (uint32_t i = 0; i < n_add; ++i)
            if (const char* r = flow_key_refusal(add[i].key)) {
                if (why) *why = "flow " + std::to_string(i) + ": " + r;
                return false;
            }
        std::map<std::string, bool> now;   // keys this update touches: present after the steps so far
        auto present = [&](const vpcsum_tuple_t& k) -> bool& {
            std::string s((const char*)&k, kFlowKeyBytes);
            auto it = now.find(s);
            if (it == now.end()) it = now.emplace(s, find(k) >= 0).first;
            return it->second;
        };
        uint64_t count = flows_;
        for (uint32_t i = 0; i < n_del; ++i) {
            bool& p = present(del[i]);
            if (p) { p = false; --count; }
        }
        for (uint32_t i = 0; i < n_add; ++i) {
            bool& p = present(add[i].key);
            if (!p) { p = true; ++count; }
        }
        if (count > max_flows_) {
            if (why) *why = "the table is full: " + std::to_string(count) + " flows > max_flows " + std::to_string(max_flows_);
            return false;
        }
        return true;
    }

    // Insert, or replace the rewrite and cookie of a key already there (its id and its Fastpath
    // stay); a new flow has no Fastpath.  The flow id, or -1 with *why set and nothing changed.
    // Slots written are noted in `dirty`.
    int64_t insert(const vpcsum_flow_t& f, FlowDirty* dirty, const char** why = nullptr) {
        if (const char* r = flow_key_refusal(f.key)) {
            if (why) *why = r;
            return -1;
        }
        const uint32_t home = (uint32_t)flow_hash(f.key) & mask_;
        uint32_t i = home;
        for (uint32_t p = 0; p < slots_; ++p, i = (i + 1) & mask_) {
            FlowSlot& s = slot_[i];
            if (s.occupied) {
                if (!flow_key_equal(s.key, f.key)) continue;
                s.rw = f.rw;
                s.cookie = f.cookie;
                cookie_[s.flow_id] = f.cookie;
                if (dirty) dirty->note(i);
                return s.flow_id;
            }
            if (flows_ >= max_flows_) break;
            uint32_t id;
            if (!free_ids_.empty()) {
                id = free_ids_.back();
                free_ids_.pop_back();
            } else {
                id = next_id_++;
            }
            memset((void*)&s, 0, sizeof(s));
            memcpy(&s.key, &f.key, kFlowKeyBytes);
            s.flow_id = id;
            s.occupied = 1;
            s.rw = f.rw;
            s.cookie = f.cookie;
            cookie_[id] = f.cookie;
            live_[id] = 1;
            ++flows_;
            add_disp(p);
            if (dirty) dirty->note(i);
            return id;
        }
        if (why) *why = "the table is full";
        return -1;
    }

    // The Fastpath of a key: 1 = set (port 0: cleared, the slot's record all zeros), 0 = the key is
    // not there, -1 = a malformed key (*why set); nothing changes unless 1.  Allocates nothing.
    int set_fastpath(const vpcsum_tuple_t& key, const vpcsum_fastpath_t& fp, FlowDirty* dirty, const char** why = nullptr) {
        if (const char* r = flow_key_refusal(key)) {
            if (why) *why = r;
            return -1;
        }
        const int64_t at = find(key);
        if (at < 0) return 0;
        FlowSlot& s = slot_[at];
        if (fp.port != 0) s.fp = fp;
        else memset(&s.fp, 0, sizeof(s.fp));
        if (dirty) dirty->note((uint32_t)at);
        return 1;
    }

    // Erase by backward shift (a shifted flow's Fastpath moves with its slot, the erased one's
    // goes); the erased flow's id (now free), or -1 when the key is not there.
    int64_t erase(const vpcsum_tuple_t& key, FlowDirty* dirty) {
        const int64_t at = find(key);
        if (at < 0) return -1;
        uint32_t i = (uint32_t)at;
        const uint32_t id = slot_[i].flow_id;
        drop_disp((i - home_of(i)) & mask_);
        for (uint32_t j = i;;) {
            j = (j + 1) & mask_;
            if (!slot_[j].occupied) break;
            const uint32_t k = home_of(j);
            // an entry whose home lies cyclically in (i, j] stays where it is
            if (i <= j ? (i < k && k <= j) : (i < k || k <= j)) continue;
            drop_disp((j - k) & mask_);
            add_disp((i - k) & mask_);
            slot_[i] = slot_[j];
            if (dirty) dirty->note(i);
            i = j;
        }
        memset((void*)&slot_[i], 0, sizeof(FlowSlot));
        if (dirty) dirty->note(i);
        live_[id] = 0;
        cookie_[id] = 0;
        free_ids_.push_back(id);
        --flows_;
        return id;
    }

private:
    uint32_t home_of(uint32_t i) const { return (uint32_t)flow_hash(slot_[i].key) & mask_; }
    void add_disp(uint32_t d) {
        ++disp_[d];
        if (d > max_probe_) max_probe_ = d;
    }
    void drop_disp(uint32_t d) {
        if (--disp_[d] == 0 && d == max_probe_)
            while (max_probe_ > 0 && disp_[max_probe_] == 0) --max_probe_;
    }

    FlowSlot* slot_;
    uint32_t slots_, mask_, max_flows_, next_id_, flows_;
    std::vector<uint32_t> free_ids_;
    std::vector<uint64_t> cookie_;     // by flow id
    std::vector<uint8_t> live_;        // by flow id
    std::vector<uint32_t> disp_;       // by displacement: live entries that far from their home slot
    uint32_t max_probe_ = 0;           // the largest displacement with a live entry
};

}  // namespace vpcsum
