// kfdb.hpp -- gfx950 KeyFrameDatabase storage and scan (reference src/KeyFrameDatabase.cc).
// Every stored keyframe's BowVector lives in one device entry pool; a query scans all of them
// (see kfdb.hip).  The list logic after the scan is host work (capi_kfdb.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <unordered_map>
#include <vector>

namespace orbgpu {

constexpr int kKfdbMaxWords = 4096;   // per BowVector (the query's words are staged in LDS)

// Device slot: one stored keyframe's span of the entry pool.  live = 0: a hole left by erase.
struct KfdbSlot {
    int32_t id, off, len, live;
};
// One keyframe of the scored subset (words > minCommonWords), in no particular order.
struct KfdbScored {
    int32_t slot, words, first;   // shared words; index in the query of the first shared word
    float score;                  // (float)L1Scoring::score(query, keyframe)
};
struct KfdbCounts {
    int32_t max_words, n_sharing, n_scored, pad;
};
// One query of a batch (host pointers).
struct KfdbQuery {
    int nq;
    const uint32_t* word;
    const double* value;
    int n_exclude;
    const int32_t* exclude;
};

class KfDatabase {
public:
    ~KfDatabase();
    // return codes: 0 ok, -2 HIP error, -3 beyond the int32 entry offsets, -4 no device
    int init(int slots, int entries);
    bool has(int32_t id) const { return slot_of_.count(id) != 0; }
    int add(int count, const int32_t* id, const int32_t* start, const uint32_t* word, const double* value);
    int erase(int32_t id);
    int clear();
    int n_keyframes() const { return (int)slot_of_.size(); }
    long long n_entries() const { return live_entries_; }
    // Scan for `count` queries: one launch set, one synchronisation.  Afterwards counts(q) and
    // scored(q)[0 .. counts(q).n_scored) are valid until the next call.
    int query(int count, const KfdbQuery* q);
    const KfdbCounts& counts(int q) const { return h_counts_[q]; }
    const KfdbScored* scored(int q) const { return h_scored_ + (size_t)q * q_stride_; }
    int32_t slot_id(int slot) const { return slots_[slot].id; }
    long long slot_seq(int slot) const { return seq_[slot]; }
    int slot_of(int32_t id) const {
        auto it = slot_of_.find(id);
        return it == slot_of_.end() ? -1 : it->second;
    }
    void enable_timing(bool on) { timing_ = on; }
    bool timed() const { return timed_; }
    float ms_share() const { return ms_[0]; }
    float ms_score() const { return ms_[1]; }

private:
    int repack(long long new_cap);
    int reserve_query(int count, size_t stage_bytes);

    hipStream_t s_ = nullptr;
    // slot table: host mirror (uploaded when dirty) + sequence numbers + free list
    std::vector<KfdbSlot> slots_;
    std::vector<long long> seq_;
    std::vector<int> free_;
    std::unordered_map<int32_t, int> slot_of_;
    KfdbSlot* d_slots_ = nullptr;
    int slot_cap_ = 0;
    bool slots_dirty_ = false;
    long long next_seq_ = 0;
    // entry pool
    uint32_t* d_word_ = nullptr;
    double* d_value_ = nullptr;
    long long pool_cap_ = 0, pool_used_ = 0, live_entries_ = 0;
    // query work area (grown on demand, kept)
    uint8_t* h_stage_ = nullptr;   // pinned: descriptors | words | excluded ids | values
    uint8_t* d_stage_ = nullptr;
    size_t stage_cap_ = 0;
    int32_t* d_work_ = nullptr;    // words | first | scored slot, each q_cap x q_stride
    KfdbCounts* d_counts_ = nullptr;
    KfdbCounts* h_counts_ = nullptr;   // pinned
    KfdbScored* h_scored_ = nullptr;   // pinned, written by k_kfdb_score
    int q_cap_ = 0, q_stride_ = 0;
    bool timing_ = false, timed_ = false;
    hipEvent_t ev_[3] = {};
    float ms_[2] = {};
};

}  // namespace orbgpu
