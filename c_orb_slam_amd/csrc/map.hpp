// map.hpp -- gfx950 Map: the keyframe <-> map-point observation relation in device memory, the
// covisibility vote over it, and Tracking::UpdateLocalMap (see map.hip).  Reference
// src/Tracking.cc:1195-1339 (UpdateLocalMap / UpdateLocalPoints / UpdateLocalKeyFrames) and
// src/KeyFrame.cc (UpdateConnections).  The list logic of UpdateConnections after the vote is
// host work (capi_map.cpp).
//
// Per live keyframe the handle stores one row: mp[slot] = the map-point id of
// KeyFrame::mvpMapPoints[slot] (-1 = none) and observed[slot] = whether that point's
// mObservations holds (keyframe, slot).  The vote reads the observed slots only;
// UpdateLocalPoints reads every slot.
//
// Id order stands in for address order: where the reference iterates a std::map<KeyFrame*, ..>
// or std::set<KeyFrame*> (keyframeCounter, KFcounter, mspChildrens) the order is the address
// order of the keyframes; here it is ascending keyframe id, and children are kept ascending.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <unordered_map>
#include <vector>

namespace orbgpu {

constexpr int kMapMaxRow = 4096;      // slots per keyframe row (the frame keypoint limit)
constexpr int kMapBest = 10;          // GetBestCovisibilityKeyFrames(10)
constexpr int kMapKfStop = 80;        // Tracking.cc:1290
constexpr int kMapLdsSlots = 8192;    // vote counters in LDS up to this many keyframe slots (32 KiB)
constexpr int kMapDefaultChunk = 64;  // frames per launch set of UpdateLocalMap
constexpr size_t kMapScratchBytes = (size_t)256 << 20;   // first-occurrence scratch of a chunk
constexpr uint8_t kMapKeyStereo = 1, kMapKeyFar = 2;     // per-cell key flags

struct MapSlotDev {
    int32_t id, off, n, live;   // row = [off, off + n) of the cell pools
};
struct MapNbDev {
    int32_t cov[kMapBest];
    int32_t ncov, parent, child_off, nchild;   // ids; children in the child pool, ascending
};
struct MapCounts {
    int32_t n_kf, ref_kf, n_pt, pad;
};
// one vote query: a list of map-point ids with multiplicity
struct MapQueryDev {
    int32_t* list;        // entries < 0 are skipped; bad entries are written back as -1
    const uint8_t* bad;   // the map-point table's isBad() flags, or null
    int32_t n, nbad;
    int32_t exclude;      // keyframe slot that gets no vote (UpdateConnections: the keyframe itself), or -1
    int32_t pad;
};
// one frame of Tracking::UpdateLocalMap (device pointers)
struct MapLocalDev {
    MapQueryDev q;        // list = mCurrentFrame.mvpMapPoints as global ids
    int32_t kf_cap, pt_cap;
    int32_t* local_kf;    // out kf_cap: mvpLocalKeyFrames (ids)
    int32_t* local_mp;    // out pt_cap: mvpLocalMapPoints (global ids)
    int32_t* cur_row;     // out q.n: local row of cur_mp[i], or -1
    int32_t* row;         // out pt_cap or null: row[j] = local_mp[j] (-1 in the padding)
    // gather of the global table's rows (all null: none)
    const float* t_pos;
    const uint8_t* t_desc;
    const int* t_obs;
    const float* t_maxd;
    const float* t_mind;
    const float* t_normal;
    int32_t t_n, pad_rows;   // pad_rows: rows [n_pt, pt_cap) get row = -1 / skip = 1
    float* g_pos;
    uint8_t* g_desc;
    int* g_obs;
    float* g_maxd;
    float* g_mind;
    float* g_normal;
    uint8_t* g_skip;
    MapCounts* counts;    // out
};
// one LocalMapping::KeyFrameCulling call (host pointers)
struct MapKfCull {
    int n;
    const int32_t* cand;        // keyframe ids in GetVectorCovisibleKeyFrames order
    const uint8_t* not_erase;   // n or null: KeyFrame::mbNotErase
    int monocular;
    const uint8_t* bad;         // the map-point table's isBad() flags, or null
    int nbad, cap_bad;
    int32_t* nMPs;              // out n
    int32_t* nRedundant;        // out n
    int32_t* verdict;           // out n
    int32_t* bad_mp;            // out cap_bad
    int n_bad;                  // out
};
// one LocalMapping::MapPointCulling call (host pointers)
struct MapPtCull {
    int n;
    const int32_t* mp;
    const int32_t* first_kf;
    const int32_t* found;
    const int32_t* visible;
    const uint8_t* bad;
    int nbad;
    int32_t cur_kf;
    int monocular;
    int32_t* verdict;           // out n
    int32_t* observations;      // out n or null
};

// the handle's device state as another unit's kernels read it (Map::begin_view)
struct MapView {
    const MapSlotDev* slots;
    const int32_t* mp;          // cell pools: map-point id, observed, octave
    const uint8_t* obs;
    const uint8_t* oct;
    const int32_t* pt_start;    // npts + 1
    const uint32_t* pt_obs;     // per point the observing cells, slot * 4096 + index, in no order
    int32_t npts;
};

class Map {
public:
    ~Map();
    // return codes: 0 ok, -1 invalid, -2 HIP error, -3 beyond the int32 cell offsets, -4 no device
    int init(int slots, int cells, int points);
    bool has(int32_t id) const { return slot_of_.count(id) != 0; }
    int slot_of(int32_t id) const {
        auto it = slot_of_.find(id);
        return it == slot_of_.end() ? -1 : it->second;
    }
    int32_t slot_id(int slot) const { return slots_[slot].id; }
    int n_slots() const { return (int)slots_.size(); }
    int n_keyframes() const { return (int)slot_of_.size(); }
    long long n_cells() const { return live_cells_; }
    long long n_observed() const { return n_observed_; }

    // mutations: host mirror only; the next query uploads what changed and rebuilds the index
    int add_keyframe(int32_t id, int N, const int32_t* mp, const uint8_t* observed);
    int set_matches(int32_t id, int count, const int32_t* slot, const int32_t* mp, const uint8_t* observed);
    int erase_point(int32_t mp);
    int replace_point(int32_t mp, int32_t by);
    int erase_keyframe(int32_t id);
    int set_neighbours(int32_t id, int n10, const int32_t* ids10, int32_t parent, int nchild,
                       const int32_t* children);
    int clear();
    // The per-slot key attributes of one row: octave, stereo (uRight >= 0) and far (depth > thDepth
    // or depth < 0).  uRight null: all monocular; depth null: no slot far.  Host mirror only.
    int set_keys(int32_t id, int N, const uint8_t* octave, const float* uRight, const float* depth, float thDepth);

    // LocalMapping::KeyFrameCulling / MapPointCulling on the handle's stream, synchronous; the
    // handle itself is not changed (the caller applies the erasures to the mirror).
    int cull_keyframes(MapKfCull& c);
    int cull_points(const MapPtCull& c);

    // The vote of `count` stored keyframes' own rows (KeyFrame::UpdateConnections), on the
    // handle's stream, synchronous: afterwards votes(q)[slot] is valid until the next call.
    int vote_rows(int count, const int32_t* ids);
    const int32_t* votes(int q) const { return h_votes_.data() + (size_t)q * n_slots(); }

    // Tracking::UpdateLocalMap for `count` frames queued on `s`; d_frames = the frames in device
    // memory (valid until the work is done), h_frames = the same on the host.
    int update_local(hipStream_t s, int count, const MapLocalDev* d_frames, const MapLocalDev* h_frames);

    // The relation for the kernels of another unit (loopcorrect.hip), on stream `s`: the stream is
    // ordered behind the handle's last query, the device state brought up to date (rows, inverse
    // index, octaves and the point -> cells index), and `v` filled.  end_view(s) closes the query.
    int begin_view(hipStream_t s, MapView& v);
    int end_view(hipStream_t s) { return leave(s); }
    int n_ids() const { return nid_; }   // largest keyframe id seen + 1
    int row_size(int slot) const { return slots_[slot].n; }
    const std::vector<int32_t>& children(int slot) const { return nb_[slot].children; }
    // a keyframe that is its own descendant over the live keyframes' children lists
    bool children_cyclic() const;
    // the host mirror of one live row, read only (capi_fuse.cpp works on a copy of what it changes)
    bool slot_live(int slot) const { return slots_[slot].live != 0; }
    const int32_t* row_mp(int slot) const { return h_mp_.data() + slots_[slot].off; }
    const uint8_t* row_obs(int slot) const { return h_obs_.data() + slots_[slot].off; }
    const uint8_t* row_oct(int slot) const { return h_oct_.data() + slots_[slot].off; }
    const uint8_t* row_flags(int slot) const { return h_flags_.data() + slots_[slot].off; }
    // the cells (slot * kMapMaxRow + index) that hold map point `mp`, in no order; null: none
    const std::vector<uint32_t>* cells_of(int32_t mp) const {
        auto it = held_.find(mp);
        return it == held_.end() ? nullptr : &it->second;
    }
    bool timing_on() const { return timing_; }

    void set_chunk(int frames) { chunk_ = frames; }
    void set_lds_slots(int n) { lds_slots_ = n; }
    void enable_timing(bool on) { timing_ = on; }
    // ms5 = rebuild, vote, keyframe selection, local points, remap + gather (HIP events of the
    // last update_local; of its last chunk where it ran several); -1 = the stage did not run
    int timings(float* ms5);

private:
    struct Nb {
        int ncov = 0;
        int32_t cov[kMapBest] = {};
        int32_t parent = -1;
        std::vector<int32_t> children;
    };
    void set_cell(int slot, int idx, int32_t mp, uint8_t obs);
    bool row_holds(int slot, int32_t mp, int except_idx) const;
    void mark_row(int slot);
    int repack(long long new_cap);
    int sync_device(hipStream_t s);        // uploads + CSR rebuild
    int sync_cull(hipStream_t s);          // key attributes + the cell index and nObs, when stale
    int join(hipStream_t s);               // order `s` behind the last query of another stream
    int leave(hipStream_t s);
    int reserve_work(int chunk);
    int drain();                           // host wait for the last query (before freeing)

    hipStream_t s_ = nullptr;
    // host mirror
    std::vector<MapSlotDev> slots_;
    std::vector<Nb> nb_;
    std::vector<int> free_;
    std::unordered_map<int32_t, int> slot_of_;
    std::vector<int32_t> h_mp_;
    std::vector<uint8_t> h_obs_;
    std::vector<uint8_t> h_oct_;     // mvKeysUn[slot].octave, beside h_mp_ / h_obs_
    std::vector<uint8_t> h_flags_;   // kMapKeyStereo | kMapKeyFar
    std::unordered_map<int32_t, std::vector<uint32_t>> held_;   // map point -> cells (slot * 4096 + idx)
    long long pool_cap_ = 0, pool_used_ = 0, live_cells_ = 0, n_observed_ = 0;
    int32_t npts_ = 0;      // largest map-point id seen + 1
    int32_t nid_ = 0;       // largest keyframe id seen + 1
    // dirty state
    std::vector<uint8_t> row_dirty_;
    std::vector<int> dirty_rows_;
    bool all_rows_dirty_ = false, meta_dirty_ = false, index_dirty_ = false;
    // device
    MapSlotDev* d_slots_ = nullptr;
    MapNbDev* d_nb_ = nullptr;
    int32_t* d_order_ = nullptr;
    int slot_cap_ = 0;
    int32_t* d_child_ = nullptr;
    int child_cap_ = 0;
    int32_t* d_id2slot_ = nullptr;
    int id_cap_ = 0;
    int32_t* d_mp_ = nullptr;
    uint8_t* d_obs_ = nullptr;
    int32_t* d_pt_list_ = nullptr;
    long long dev_pool_cap_ = 0;
    int32_t* d_pt_start_ = nullptr;    // npts + 1
    int32_t* d_pt_cursor_ = nullptr;   // npts + 1
    int pt_cap_ = 0;
    int n_live_dev_ = 0;
    // culling: built only when a culling call follows a mutation (sync_cull)
    bool cull_dirty_ = true;
    uint8_t* d_oct_ = nullptr;         // cell pools beside d_mp_ / d_obs_
    uint8_t* d_flags_ = nullptr;
    uint32_t* d_pt_obs_ = nullptr;     // per point, the observing cells as slot * 4096 + index (CSR over d_pt_start_)
    long long cull_pool_cap_ = 0;
    int32_t* d_nobs_ = nullptr;        // per point MapPoint::nObs: 2 per stereo observation, 1 per monocular
    int32_t* d_cull_scr_ = nullptr;    // per point, zeroed per call: what the call's culls took off nObs | kCullBad
    int cull_pt_cap_ = 0;
    uint8_t* d_dead_ = nullptr;        // per keyframe slot, zeroed per call: culled by this call
    int cull_slot_cap_ = 0;
    uint8_t* d_cull_io_ = nullptr;     // the arguments and results of one call
    size_t cull_io_cap_ = 0;
    // work area of a chunk
    int32_t* d_work_ = nullptr;        // cnt | kfslot | rowcnt | rowoff, each chunk x stride
    int32_t* d_scr_ = nullptr;         // chunk x scr_stride, INT_MAX when idle
    MapCounts* d_counts_ = nullptr;    // vote_rows only
    MapQueryDev* d_q_ = nullptr;       // vote_rows only
    int work_chunk_ = 0, work_stride_ = 0, scr_stride_ = 0;
    std::vector<int32_t> h_votes_;
    int chunk_ = 0, lds_slots_ = -1;
    // ordering between the streams that query the handle
    hipEvent_t ev_done_ = nullptr;
    hipStream_t last_stream_ = nullptr;
    bool ev_recorded_ = false;
    bool timing_ = false, timed_ = false, timed_rebuild_ = false;
    hipEvent_t ev_[7] = {};
};

}  // namespace orbgpu
