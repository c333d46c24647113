// capi_loopcorrect.cpp -- extern "C" LoopClosing_CorrectLoop and LoopClosing_ApplyGlobalBA
// (include/orbslam_gpu.h), reference src/LoopClosing.cc (CorrectLoop, RunGlobalBundleAdjustment).
// Argument checks, the processing order, the spanning-tree levels (from the handle's host
// mirror) and the pointer-space staging are here; the arithmetic runs in loopcorrect.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <numeric>
#include <utility>
#include <vector>

#include "../../include/orbslam_gpu.h"
#include "capi_handles.hpp"
#include "loopcorrect.hpp"

namespace {

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

int no_handle() { return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID; }

size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

// The tables of one call: in device-pointer mode the caller's arrays themselves, otherwise
// copies in the matcher's arena that go up before the kernels and come back after them.
class Tables {
public:
    Tables(orbgpu::Matcher* m, bool dev) : m_(m), dev_(dev), s_(m->stream()) {}
    void want(const void* user, size_t bytes) {
        if (!dev_ && user) need_ += al256(bytes);
    }
    void want_work(size_t bytes) { need_ += al256(std::max(bytes, (size_t)1)); }
    int reserve() { return m_->arena_reserve(need_ + 256); }
    // in (and in/out) table array; out: copied back by download()
    template <class T>
    T* table(T* user, size_t bytes, bool out) {
        if (dev_ || !user || bytes == 0) return user;
        void* d = m_->arena_alloc(bytes);
        if (!d || hipMemcpyAsync(d, user, bytes, hipMemcpyHostToDevice, s_) != hipSuccess) {
            fail_ = true;
            return nullptr;
        }
        if (out) back_.push_back({(void*)user, d, bytes});
        return (T*)d;
    }
    template <class T>
    T* work(size_t count) {
        void* d = m_->arena_alloc(sizeof(T) * std::max(count, (size_t)1));
        if (!d) fail_ = true;
        return (T*)d;
    }
    template <class T>
    T* upload(const T* host, size_t count) {
        T* d = work<T>(count);
        if (d && count && hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, s_) != hipSuccess) fail_ = true;
        return d;
    }
    bool failed() const { return fail_; }
    bool download() {
        for (const Back& b : back_)
            if (hipMemcpyAsync(b.user, b.dev, b.bytes, hipMemcpyDeviceToHost, s_) != hipSuccess) return false;
        return true;
    }

private:
    struct Back {
        void* user;
        void* dev;
        size_t bytes;
    };
    orbgpu::Matcher* m_;
    bool dev_;
    hipStream_t s_;
    size_t need_ = 0;
    bool fail_ = false;
    std::vector<Back> back_;
};

}  // namespace

extern "C" {

int LoopClosing_CorrectLoop(ORBmatcher_h mh, Map_h h, orb_loopcorrect* C) {
    if (!C || C->nkf <= 0 || !C->kf || !C->Scw || C->nlevels <= 0 || !C->scale_factors || C->n_kf_rows <= 0 ||
        !C->Tcw || !C->CorrectedSim3 || !C->NonCorrectedSim3)
        return ORB_E_INVALID;
    const orb_pointtable& T = C->pts;
    if (T.n < 0) return ORB_E_INVALID;
    if (T.n > 0 && (!T.pos || !T.normal || !T.max_dist || !T.min_dist || !T.ref_kf || !C->corrected_ref))
        return ORB_E_INVALID;
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(C->Scw[k])) return ORB_E_INVALID;
    if (!(C->Scw[7] > 0)) return ORB_E_INVALID;
    const int nkf = C->nkf;
    // processing order: ascending id (the id-order rule for the KeyFrameAndPose map)
    std::vector<int> order((size_t)nkf);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return C->kf[a] < C->kf[b]; });
    int cur = -1;
    for (int j = 0; j < nkf; j++) {
        const int32_t id = C->kf[order[j]];
        if (id < 0 || id >= C->n_kf_rows) return ORB_E_INVALID;
        if (j > 0 && id == C->kf[order[j - 1]]) return ORB_E_INVALID;
        if (id == C->cur_kf) cur = j;
    }
    if (cur < 0) return ORB_E_INVALID;
    if (!mh || !h) return no_handle();
    orbgpu::Matcher* m = mh->m;
    if (m->chain().on()) return ORB_E_INVALID;
    const bool dev = m->device_pointers();
    hipStream_t s = m->stream();
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->map.n_ids() > C->n_kf_rows) return ORB_E_INVALID;
    std::vector<int32_t> ids((size_t)nkf), slots((size_t)nkf);
    int max_row = 0;
    for (int j = 0; j < nkf; j++) {
        ids[j] = C->kf[order[j]];
        slots[j] = h->map.slot_of(ids[j]);
        if (slots[j] < 0) return ORB_E_INVALID;
        max_row = std::max(max_row, h->map.row_size(slots[j]));
    }
    if (h->map.children_cyclic()) return ORB_E_INVALID;

    orbgpu::LoopCorrectDev D;
    std::memset(&D, 0, sizeof(D));
    if (int e = h->map.begin_view(s, D.V)) return e == -4 ? ORB_E_NODEVICE : ORB_E_HIP;
    const size_t np = (size_t)T.n, nr = (size_t)C->n_kf_rows;
    Tables tab(m, dev);
    tab.want(C->Tcw, nr * 64);
    tab.want(T.pos, np * 12);
    tab.want(T.normal, np * 12);
    tab.want(T.max_dist, np * 4);
    tab.want(T.min_dist, np * 4);
    tab.want(T.bad, np);
    tab.want(T.ref_kf, np * 4);
    tab.want(C->corrected_ref, np * 4);
    tab.want_work(4 * (size_t)nkf);          // ids
    tab.want_work(4 * (size_t)nkf);          // slots
    tab.want_work(64);                       // Scw
    tab.want_work(4 * (size_t)C->nlevels);   // scale factors
    tab.want_work(4 * nr);                   // proc
    tab.want_work(4 * np);                   // claim
    tab.want_work(3 * 64 * (size_t)nkf);     // corr | noncorr | corr_inv
    tab.want_work(64 * (size_t)nkf);         // newT
    tab.want_work(12 * (size_t)nkf);         // newOw
    tab.want_work(8);                        // counts
    if (tab.reserve()) return ORB_E_HIP;
    D.nkf = nkf;
    D.cur = cur;
    D.nlevels = C->nlevels;
    D.n_kf_rows = C->n_kf_rows;
    D.n_pt_rows = T.n;
    D.Tcw = tab.table(C->Tcw, nr * 64, true);
    D.pos = tab.table(T.pos, np * 12, true);
    D.normal = tab.table(T.normal, np * 12, true);
    D.max_dist = tab.table(T.max_dist, np * 4, true);
    D.min_dist = tab.table(T.min_dist, np * 4, true);
    D.bad = tab.table(T.bad, np, false);
    D.ref_kf = tab.table(T.ref_kf, np * 4, false);
    D.corrected_ref = tab.table(C->corrected_ref, np * 4, true);
    D.kf_id = tab.upload(ids.data(), (size_t)nkf);
    D.kf_slot = tab.upload(slots.data(), (size_t)nkf);
    D.Scw = tab.upload(C->Scw, 8);
    D.scale = tab.upload(C->scale_factors, (size_t)C->nlevels);
    D.proc = tab.work<int32_t>(nr);
    D.claim = tab.work<int32_t>(np);
    D.corr = tab.work<double>(3 * 8 * (size_t)nkf);
    D.newT = tab.work<float>(16 * (size_t)nkf);
    D.newOw = tab.work<float>(3 * (size_t)nkf);
    D.counts = tab.work<int32_t>(2);
    if (tab.failed()) return ORB_E_HIP;
    D.noncorr = D.corr + 8 * (size_t)nkf;
    D.corr_inv = D.corr + 16 * (size_t)nkf;
    if (hipMemsetAsync(D.proc, 0xff, 4 * nr, s) != hipSuccess) return ORB_E_HIP;
    if (np && hipMemsetAsync(D.claim, orbgpu::kLoopClaimIdleByte, 4 * np, s) != hipSuccess) return ORB_E_HIP;
    if (hipMemsetAsync(D.counts, 0, 8, s) != hipSuccess) return ORB_E_HIP;
    if (orbgpu::loop_correct_launch(D, max_row, s)) return ORB_E_HIP;
    std::vector<double> sims(16 * (size_t)nkf);
    int32_t counts[2] = {0, 0};
    if (hipMemcpyAsync(sims.data(), D.corr, 8 * sims.size(), hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
    if (hipMemcpyAsync(counts, D.counts, 8, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
    if (!tab.download()) return ORB_E_HIP;
    if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    if (h->map.end_view(s)) return ORB_E_HIP;
    for (int j = 0; j < nkf; j++) {
        std::memcpy(C->CorrectedSim3 + 8 * (size_t)order[j], sims.data() + 8 * (size_t)j, 64);
        std::memcpy(C->NonCorrectedSim3 + 8 * (size_t)order[j], sims.data() + 8 * ((size_t)nkf + j), 64);
    }
    C->n_corrected = counts[0];
    C->n_ref_missing = counts[1];
    return ORB_OK;
}

int LoopClosing_ApplyGlobalBA(ORBmatcher_h mh, Map_h h, orb_gbaapply* G) {
    if (!G || G->norigins < 0 || (G->norigins > 0 && !G->origins) || G->n_kf_rows <= 0 || !G->TcwGBA ||
        !G->kf_in_gba || !G->Tcw)
        return ORB_E_INVALID;
    const orb_pointtable& T = G->pts;
    if (T.n < 0) return ORB_E_INVALID;
    if (T.n > 0 && (!T.pos || !T.ref_kf || !G->posGBA || !G->mp_in_gba)) return ORB_E_INVALID;
    for (int i = 0; i < G->norigins; i++)
        if (G->origins[i] < 0 || G->origins[i] >= G->n_kf_rows) return ORB_E_INVALID;
    if (!mh || !h) return no_handle();
    orbgpu::Matcher* m = mh->m;
    if (m->chain().on()) return ORB_E_INVALID;
    const bool dev = m->device_pointers();
    hipStream_t s = m->stream();
    std::lock_guard<std::mutex> lk(h->mu);
    orbgpu::Map& map = h->map;
    if (map.n_ids() > G->n_kf_rows) return ORB_E_INVALID;
    if (map.children_cyclic()) return ORB_E_INVALID;
    const size_t np = (size_t)T.n, nr = (size_t)G->n_kf_rows;
    std::vector<uint8_t> in_gba(nr);
    if (dev) {
        if (hipMemcpyAsync(in_gba.data(), G->kf_in_gba, nr, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    } else {
        std::memcpy(in_gba.data(), G->kf_in_gba, nr);
    }
    // breadth first over the host mirror; step[id] = the un-optimised keyframes on the path down
    // to and including id since the last optimised one: the dependent step that computes its pose
    std::vector<uint8_t> reached(nr, 0);
    std::vector<int32_t> step(nr, 0), queue;
    std::vector<std::vector<int32_t>> levels;
    for (int i = 0; i < G->norigins; i++) {
        const int32_t o = G->origins[i];
        if (!map.has(o) || reached[o]) continue;
        if (!in_gba[o]) return ORB_E_INVALID;
        reached[o] = 1;
        queue.push_back(o);
    }
    int n_prop = 0;
    for (size_t q = 0; q < queue.size(); q++) {
        const int32_t id = queue[q];
        for (int32_t c : map.children(map.slot_of(id))) {
            if (!map.has(c) || reached[c]) continue;
            reached[c] = 1;
            if (!in_gba[c]) {
                step[c] = step[id] + 1;
                if ((int)levels.size() < step[c]) levels.resize((size_t)step[c]);
                levels[(size_t)step[c] - 1].push_back(c);
                levels[(size_t)step[c] - 1].push_back(id);
                n_prop++;
            }
            queue.push_back(c);
        }
    }
    const int depth = (int)levels.size();
    std::vector<int32_t> pairs;
    std::vector<int> level_off((size_t)depth + 1, 0);
    for (int l = 0; l < depth; l++) {
        pairs.insert(pairs.end(), levels[l].begin(), levels[l].end());
        level_off[(size_t)l + 1] = (int)(pairs.size() / 2);
    }

    Tables tab(m, dev);
    tab.want(G->Tcw, nr * 64);
    tab.want(G->TcwGBA, nr * 64);
    tab.want(G->TcwBefGBA, nr * 64);
    tab.want(T.pos, np * 12);
    tab.want(G->posGBA, np * 12);
    tab.want(G->mp_in_gba, np);
    tab.want(T.bad, np);
    tab.want(T.ref_kf, np * 4);
    tab.want_work(nr);                 // reached
    tab.want_work(4 * pairs.size());   // pairs
    tab.want_work(8);                  // counts
    if (tab.reserve()) return ORB_E_HIP;
    orbgpu::GbaApplyDev D;
    std::memset(&D, 0, sizeof(D));
    D.n_kf_rows = G->n_kf_rows;
    D.n_pt_rows = T.n;
    D.Tcw = tab.table(G->Tcw, nr * 64, true);
    D.TcwGBA = tab.table(G->TcwGBA, nr * 64, true);
    // host mode: the rows of unreached keyframes come back as they went up
    D.TcwBef = tab.table(G->TcwBefGBA, nr * 64, true);
    D.pos = tab.table(T.pos, np * 12, true);
    D.posGBA = tab.table(G->posGBA, np * 12, false);
    D.mp_in_gba = tab.table(G->mp_in_gba, np, false);
    D.bad = tab.table(T.bad, np, false);
    D.ref_kf = tab.table(T.ref_kf, np * 4, false);
    D.reached = tab.upload(reached.data(), nr);
    D.pair = tab.upload(pairs.data(), pairs.size());
    D.counts = tab.work<int32_t>(2);
    if (tab.failed()) return ORB_E_HIP;
    if (hipMemsetAsync(D.counts, 0, 8, s) != hipSuccess) return ORB_E_HIP;
    if (orbgpu::gba_apply_launch(D, depth, level_off.data(), s)) return ORB_E_HIP;
    int32_t counts[2] = {0, 0};
    if (hipMemcpyAsync(counts, D.counts, 8, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
    if (!tab.download()) return ORB_E_HIP;
    if (G->kf_done) {
        if (dev) {
            if (hipMemcpyAsync(G->kf_done, D.reached, nr, hipMemcpyDeviceToDevice, s) != hipSuccess) return ORB_E_HIP;
        } else {
            std::memcpy(G->kf_done, reached.data(), nr);
        }
    }
    if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    G->n_kf_propagated = n_prop;
    G->n_mp_gba = counts[0];
    G->n_mp_moved = counts[1];
    G->depth = depth;
    return ORB_OK;
}

}  // extern "C"
