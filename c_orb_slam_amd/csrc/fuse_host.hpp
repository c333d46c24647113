// fuse_host.hpp -- the host side that LocalMapping_SearchInNeighbors (capi_fuse.cpp) and
// LoopClosing_SearchAndFuse (capi_loopfuse.cpp) share: the copy-on-write image of the Map handle's
// relation the passes replay their mutations on, the bump allocator over a FuseWork buffer and the
// HIP-event pairs around the stages of one call.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "fuse.hpp"
#include "map.hpp"

namespace orbgpu {
namespace fuse_host {

inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

// The relation as the passes see it: the handle's host mirror with the rows and the point -> cells
// lists this call changed kept beside it.  set_cell / row_holds / replace follow map.hip's.
class WorkRel {
public:
    // npts: the table's rows; every point id the passes touch is below it (checked by the caller)
    WorkRel(const Map& m, size_t npts) : M(m), rows_((size_t)m.n_slots()), cells_(npts), loaded_(npts, 0) {}
    int32_t mp(int sl, int idx) const {
        const Row& R = rows_[(size_t)sl];
        return R.own ? R.mp[(size_t)idx] : M.row_mp(sl)[idx];
    }
    bool observed(int sl, int idx) const {
        const Row& R = rows_[(size_t)sl];
        return (R.own ? R.obs[(size_t)idx] : M.row_obs(sl)[idx]) != 0;
    }
    std::vector<uint32_t>& cells(int32_t p) {
        std::vector<uint32_t>& v = cells_[(size_t)p];
        if (!loaded_[(size_t)p]) {
            loaded_[(size_t)p] = 1;
            if (const std::vector<uint32_t>* c = M.cells_of(p)) v = *c;
        }
        return v;
    }
    void set_cell(int sl, int idx, int32_t p, bool obs) {
        Row& R = row(sl);
        const uint32_t code = (uint32_t)sl * kMapMaxRow + (uint32_t)idx;
        const int32_t old = R.mp[(size_t)idx];
        if (old >= 0 && old != p) {
            std::vector<uint32_t>& v = cells(old);
            for (size_t k = 0; k < v.size(); k++)
                if (v[k] == code) {
                    v[k] = v.back();
                    v.pop_back();
                    break;
                }
        }
        if (p >= 0 && old != p) cells(p).push_back(code);
        R.mp[(size_t)idx] = p;
        R.obs[(size_t)idx] = p >= 0 && obs;
    }
    bool row_holds(int sl, int32_t p) {
        for (uint32_t c : cells(p))
            if ((int)(c / kMapMaxRow) == sl) return true;
        return false;
    }
    // MapPoint::Replace as Map_ReplaceMapPoint
    void replace(int32_t p, int32_t by) {
        if (p == by) return;
        const std::vector<uint32_t> cs = cells(p);
        for (uint32_t c : cs) {
            const int sl = (int)(c / kMapMaxRow), idx = (int)(c % kMapMaxRow);
            if (observed(sl, idx) && !row_holds(sl, by)) set_cell(sl, idx, by, true);
            else set_cell(sl, idx, -1, false);
        }
    }
    // MapPoint::Observations(): 2 per stereo observation, 1 per monocular one
    int nobs(int32_t p) {
        int n = 0;
        for (uint32_t c : cells(p)) {
            const int sl = (int)(c / kMapMaxRow), idx = (int)(c % kMapMaxRow);
            if (observed(sl, idx)) n += (M.row_flags(sl)[idx] & orbgpu::kMapKeyStereo) ? 2 : 1;
        }
        return n;
    }
    // mObservations in ascending keyframe id: (id, slot * kMapMaxRow + index)
    void observers(int32_t p, std::vector<std::pair<int32_t, uint32_t>>& out) {
        out.clear();
        for (uint32_t c : cells(p)) {
            const int sl = (int)(c / kMapMaxRow);
            if (observed(sl, (int)(c % kMapMaxRow))) out.emplace_back(M.slot_id(sl), c);
        }
        std::sort(out.begin(), out.end());
    }

private:
    struct Row {
        bool own = false;
        std::vector<int32_t> mp;
        std::vector<uint8_t> obs;
    };
    Row& row(int sl) {
        Row& R = rows_[(size_t)sl];
        if (!R.own) {
            const int n = M.row_size(sl);
            R.mp.assign(M.row_mp(sl), M.row_mp(sl) + n);
            R.obs.assign(M.row_obs(sl), M.row_obs(sl) + n);
            R.own = true;
        }
        return R;
    }
    const Map& M;
    std::vector<Row> rows_;                       // by handle slot: the rows this call changed
    std::vector<std::vector<uint32_t>> cells_;    // by point: its cells, loaded from the handle on first use
    std::vector<uint8_t> loaded_;
};

struct Bump {
    char* base = nullptr;
    size_t used = 0, cap = 0;
    template <class T>
    T* take(size_t count) {
        const size_t b = al(std::max(count, (size_t)1) * sizeof(T));
        if (!base || used + b > cap) return nullptr;
        T* p = (T*)(base + used);
        used += b;
        return p;
    }
};

// HIP-event pairs around the stages of one call, summed per stage afterwards
struct StageTimer {
    orbgpu::FuseWork& W;
    hipStream_t s;
    bool on;
    std::vector<int> stage;   // stage of pair k: events 2k, 2k + 1
    bool ok = true;
    void begin(int st) {
        if (!on) return;
        hipEvent_t e = W.event(2 * stage.size());
        ok = ok && e && hipEventRecord(e, s) == hipSuccess;
        stage.push_back(st);
    }
    void end() {
        if (!on) return;
        hipEvent_t e = W.event(2 * stage.size() - 1);
        ok = ok && e && hipEventRecord(e, s) == hipSuccess;
    }
    void finish(double replay_ms) {
        W.timed = false;
        if (!on || !ok) return;
        float ms[5] = {0.f, 0.f, 0.f, 0.f, (float)replay_ms};
        for (size_t k = 0; k < stage.size(); k++) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, W.ev[2 * k], W.ev[2 * k + 1]) != hipSuccess) return;
            ms[stage[k]] += t;
        }
        std::memcpy(W.ms, ms, sizeof(ms));
        W.timed = true;
    }
};

}  // namespace fuse_host
}  // namespace orbgpu
