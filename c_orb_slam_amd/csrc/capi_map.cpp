// capi_map.cpp -- extern "C" Map_*, KeyFrame_UpdateConnections[_batch] and
// Tracking_UpdateLocalMap_batch (include/orbslam_gpu.h), reference src/Tracking.cc:1195-1339,
// src/KeyFrame.cc (UpdateConnections), src/MapPoint.cc (SetBadFlag, Replace).
// The mutations update the handle's host mirror; the vote and UpdateLocalMap run on the device
// (map.hip).  UpdateConnections downloads the vote once and builds KFcounter and the ordered
// list here, in the reference's order.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/orbslam_gpu.h"
#include "capi_handles.hpp"
#include "map.hpp"

namespace {

constexpr int kDefaultSlots = 1024, kDefaultCells = 1 << 20, kDefaultPoints = 1 << 16;
// orbgpu_unit_set_map_initial_capacity / _chunk / _lds_slots
std::atomic<int> g_init_slots{kDefaultSlots}, g_init_cells{kDefaultCells}, g_init_points{kDefaultPoints};
std::atomic<int> g_chunk{0}, g_lds_slots{-1};

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

int rc_of(int e) {
    return e == 0 ? ORB_OK : e == -1 ? ORB_E_INVALID : e == -4 ? ORB_E_NODEVICE : e == -3 ? ORB_E_CAPACITY : ORB_E_HIP;
}

int no_handle() { return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID; }

// a row holds a map point at most once (KeyFrame::mvpMapPoints of a consistent map)
bool row_unique(int n, const int32_t* mp) {
    std::unordered_set<int32_t> seen;
    for (int i = 0; i < n; i++)
        if (mp[i] >= 0 && !seen.insert(mp[i]).second) return false;
    return true;
}

void apply_knobs(Map_t* h) {
    h->map.set_chunk(g_chunk.load());
    h->map.set_lds_slots(g_lds_slots.load());
}

// KeyFrame.cc UpdateConnections over the vote of one keyframe
int finish_connections(Map_t* h, int qi, orb_connections& r) {
    const int32_t* v = h->map.votes(qi);
    const int nslots = h->map.n_slots();
    std::vector<std::pair<int32_t, int32_t>> counter;   // (id, count): KFcounter in id order
    for (int sl = 0; sl < nslots; sl++)
        if (v[sl] > 0) counter.emplace_back(h->map.slot_id(sl), v[sl]);
    std::sort(counter.begin(), counter.end());
    int nmax = 0;
    int32_t kfmax = -1;
    std::vector<std::pair<int32_t, int32_t>> vPairs;   // (weight, id)
    for (const auto& c : counter) {
        if (c.second > nmax) {
            nmax = c.second;
            kfmax = c.first;
        }
        if (c.second >= 15) vPairs.emplace_back(c.second, c.first);
    }
    if (vPairs.empty() && !counter.empty()) vPairs.emplace_back(nmax, kfmax);
    std::sort(vPairs.begin(), vPairs.end());   // ascending (weight, id); push_front reverses
    r.n_counter = (int)counter.size();
    r.n_ordered = (int)vPairs.size();
    for (int i = 0; i < std::min(r.n_counter, r.cap_counter); i++) {
        r.counter_id[i] = counter[i].first;
        r.counter_n[i] = counter[i].second;
    }
    for (int i = 0; i < std::min(r.n_ordered, r.cap_ordered); i++) {
        const auto& p = vPairs[vPairs.size() - 1 - (size_t)i];
        r.ordered_id[i] = p.second;
        r.ordered_w[i] = p.first;
    }
    return (r.n_counter > r.cap_counter || r.n_ordered > r.cap_ordered) ? ORB_E_CAPACITY : ORB_OK;
}

}  // namespace

extern "C" {

int Map_create(Map_h* out) {
    if (!out) return ORB_E_INVALID;
    *out = nullptr;
    if (no_device()) return ORB_E_NODEVICE;
    auto* h = new (std::nothrow) Map_t;
    if (!h) return ORB_E_INVALID;
    if (int e = h->map.init(g_init_slots.load(), g_init_cells.load(), g_init_points.load())) {
        delete h;
        return rc_of(e);
    }
    *out = h;
    return ORB_OK;
}

int Map_destroy(Map_h h) {
    if (!h) return ORB_E_INVALID;
    delete h;
    return ORB_OK;
}

int Map_clear(Map_h h) {
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->map.clear());
}

int Map_size(Map_h h, int* n_keyframes, long long* n_slots, long long* n_observations) {
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    if (n_keyframes) *n_keyframes = h->map.n_keyframes();
    if (n_slots) *n_slots = h->map.n_cells();
    if (n_observations) *n_observations = h->map.n_observed();
    return ORB_OK;
}

int Map_AddKeyFrame(Map_h h, int32_t id, int N, const int32_t* mp, const uint8_t* observed) {
    if (id < 0 || N < 0 || N > orbgpu::kMapMaxRow || (N > 0 && !mp)) return ORB_E_INVALID;
    if (!row_unique(N, mp)) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->map.has(id)) return ORB_E_INVALID;
    return rc_of(h->map.add_keyframe(id, N, mp, observed));
}

int Map_SetMapPointMatches(Map_h h, int32_t id, int count, const int32_t* slot, const int32_t* mp,
                           const uint8_t* observed) {
    if (id < 0 || count < 0 || (count > 0 && (!slot || !mp))) return ORB_E_INVALID;
    {
        std::unordered_set<int32_t> seen_slot, seen_mp;   // one update per slot, one slot per point
        for (int k = 0; k < count; k++) {
            if (!seen_slot.insert(slot[k]).second) return ORB_E_INVALID;
            if (mp[k] >= 0 && !seen_mp.insert(mp[k]).second) return ORB_E_INVALID;
        }
    }
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    // a point moved between two slots of the row by one call: empty the sources first
    std::vector<int32_t> none;
    std::vector<int32_t> src;
    for (int k = 0; k < count; k++)
        if (mp[k] < 0) src.push_back(slot[k]);
    if (!src.empty()) {
        none.assign(src.size(), -1);
        if (int e = h->map.set_matches(id, (int)src.size(), src.data(), none.data(), nullptr)) return rc_of(e);
    }
    return rc_of(h->map.set_matches(id, count, slot, mp, observed));
}

int Map_EraseMapPoint(Map_h h, int32_t mp) {
    if (mp < 0) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->map.erase_point(mp));
}

int Map_ReplaceMapPoint(Map_h h, int32_t mp, int32_t by) {
    if (mp < 0 || by < 0) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->map.replace_point(mp, by));
}

int Map_EraseKeyFrame(Map_h h, int32_t id) {
    if (id < 0) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->map.erase_keyframe(id));
}

int Map_SetNeighbours(Map_h h, int32_t id, int n10, const int32_t* ids10, int32_t parent, int nchild,
                      const int32_t* children) {
    if (id < 0 || n10 < 0 || n10 > orbgpu::kMapBest || (n10 > 0 && !ids10) || nchild < 0 || (nchild > 0 && !children))
        return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->map.set_neighbours(id, n10, ids10, parent, nchild, children));
}

int KeyFrame_UpdateConnections_batch(Map_h h, int count, const int32_t* id, orb_connections* r) {
    if (count < 0 || (count > 0 && (!id || !r))) return ORB_E_INVALID;
    for (int i = 0; i < count; i++)
        if (id[i] < 0 || r[i].cap_counter < 0 || r[i].cap_ordered < 0 ||
            (r[i].cap_counter > 0 && (!r[i].counter_id || !r[i].counter_n)) ||
            (r[i].cap_ordered > 0 && (!r[i].ordered_id || !r[i].ordered_w)))
            return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < count; i++)
        if (!h->map.has(id[i])) return ORB_E_INVALID;
    if (count == 0) return ORB_OK;
    apply_knobs(h);
    if (int e = h->map.vote_rows(count, id)) return rc_of(e);
    int rc = ORB_OK;
    for (int i = 0; i < count; i++)
        if (int e = finish_connections(h, i, r[i])) rc = e;
    return rc;
}

int KeyFrame_UpdateConnections(Map_h h, int32_t id, orb_connections* r) {
    if (!r) return ORB_E_INVALID;
    return KeyFrame_UpdateConnections_batch(h, 1, &id, r);
}

int Tracking_UpdateLocalMap_batch(ORBmatcher_h mh, Map_h h, int count, orb_localupdate* U) {
    if (count < 0 || (count > 0 && !U)) return ORB_E_INVALID;
    for (int f = 0; f < count; f++) {
        const orb_localupdate& u = U[f];
        if (u.N < 0 || u.N > orbgpu::kMapMaxRow || u.kf_cap < 0 || u.pt_cap < 0) return ORB_E_INVALID;
        if (u.N > 0 && (!u.cur_mp || !u.cur_row)) return ORB_E_INVALID;
        if ((u.kf_cap > 0 && !u.local_kf) || (u.pt_cap > 0 && !u.local_mp)) return ORB_E_INVALID;
        if (u.table && (u.table->n < 0 || (u.table->n > 0 && !u.table->skip))) return ORB_E_INVALID;
        const bool any = u.pos || u.desc || u.observations || u.max_dist || u.min_dist || u.normal || u.skip;
        if (any) {
            const bool all = u.pos && u.desc && u.observations && u.max_dist && u.min_dist && u.normal && u.skip;
            const orb_localmap* t = u.table;
            if (!all || !t || !t->pos || !t->desc || !t->observations || !t->max_dist || !t->min_dist || !t->normal)
                return ORB_E_INVALID;
        }
    }
    if (!mh || !h) return no_handle();
    orbgpu::Matcher* m = mh->m;
    const bool dev = m->device_pointers();
    if (!dev)
        for (int f = 0; f < count; f++)
            if (U[f].skip) return ORB_E_INVALID;   // the gather is device to device
    if (count == 0) return ORB_OK;
    hipStream_t s = m->stream();
    auto al = [](size_t n) { return (n + 255) & ~(size_t)255; };
    size_t need = al(sizeof(orbgpu::MapLocalDev) * (size_t)count) + al(sizeof(orbgpu::MapCounts) * (size_t)count) + 4096;
    if (!dev)
        for (int f = 0; f < count; f++) {
            const orb_localupdate& u = U[f];
            need += 2 * al(4 * (size_t)u.N) + al(4 * (size_t)u.kf_cap) + al(4 * (size_t)u.pt_cap) +
                    (u.table ? al((size_t)u.table->n) : 0);
        }
    if (m->arena_reserve(need)) return ORB_E_HIP;
    std::vector<orbgpu::MapLocalDev> P((size_t)count);
    orbgpu::MapCounts* d_counts = (orbgpu::MapCounts*)m->count_buf(sizeof(orbgpu::MapCounts) * (size_t)count);
    orbgpu::MapLocalDev* d_frames = (orbgpu::MapLocalDev*)m->arena_alloc(sizeof(orbgpu::MapLocalDev) * (size_t)count);
    if (!d_counts || !d_frames) return ORB_E_HIP;
    const orb_localmap* last_table = nullptr;
    const uint8_t* last_bad = nullptr;
    for (int f = 0; f < count; f++) {
        const orb_localupdate& u = U[f];
        orbgpu::MapLocalDev& d = P[f];
        std::memset(&d, 0, sizeof(d));
        d.q.n = u.N;
        d.q.exclude = -1;
        d.q.nbad = u.table ? u.table->n : 0;
        d.kf_cap = u.kf_cap;
        d.pt_cap = u.pt_cap;
        d.counts = d_counts + f;
        if (dev) {
            d.q.list = u.cur_mp;
            d.q.bad = u.table ? u.table->skip : nullptr;
            d.local_kf = u.local_kf;
            d.local_mp = u.local_mp;
            d.cur_row = u.cur_row;
            d.row = u.row;
            d.pad_rows = 1;
            if (u.skip) {
                const orb_localmap* t = u.table;
                d.t_pos = t->pos; d.t_desc = t->desc; d.t_obs = t->observations;
                d.t_maxd = t->max_dist; d.t_mind = t->min_dist; d.t_normal = t->normal;
                d.t_n = t->n;
                d.g_pos = u.pos; d.g_desc = u.desc; d.g_obs = u.observations;
                d.g_maxd = u.max_dist; d.g_mind = u.min_dist; d.g_normal = u.normal; d.g_skip = u.skip;
            }
        } else {
            d.q.list = (int32_t*)m->arena_alloc(4 * (size_t)std::max(u.N, 1));
            d.cur_row = (int32_t*)m->arena_alloc(4 * (size_t)std::max(u.N, 1));
            d.local_kf = (int32_t*)m->arena_alloc(4 * (size_t)std::max(u.kf_cap, 1));
            d.local_mp = (int32_t*)m->arena_alloc(4 * (size_t)std::max(u.pt_cap, 1));
            if (!d.q.list || !d.cur_row || !d.local_kf || !d.local_mp) return ORB_E_HIP;
            if (u.N > 0 && hipMemcpyAsync(d.q.list, u.cur_mp, 4 * (size_t)u.N, hipMemcpyHostToDevice, s) != hipSuccess)
                return ORB_E_HIP;
            if (u.table && u.table->n > 0) {
                if (u.table != last_table) {   // frames of a batch usually share one table
                    uint8_t* b = (uint8_t*)m->arena_alloc((size_t)u.table->n);
                    if (!b || hipMemcpyAsync(b, u.table->skip, (size_t)u.table->n, hipMemcpyHostToDevice, s) != hipSuccess)
                        return ORB_E_HIP;
                    last_table = u.table;
                    last_bad = b;
                }
                d.q.bad = last_bad;
            }
        }
    }
    const size_t fb = sizeof(orbgpu::MapLocalDev) * (size_t)count;
    if (hipMemcpyAsync(d_frames, m->h2d_src(P.data(), fb), fb, hipMemcpyHostToDevice, s) != hipSuccess) return ORB_E_HIP;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        apply_knobs(h);
        if (int e = h->map.update_local(s, count, d_frames, P.data())) return rc_of(e);
    }
    if (dev) {
        // n_kf, ref_kf, n_pt of every frame: now, or when the deferred chain finishes
        for (int f = 0; f < count; f++)
            if (m->d2h_counts(&U[f].n_kf, d_counts + f, sizeof(orbgpu::MapCounts))) return ORB_E_HIP;
        if (m->end_call()) return ORB_E_HIP;
        if (m->chain().on()) return ORB_OK;
    } else {
        std::vector<orbgpu::MapCounts> c((size_t)count);
        if (hipMemcpyAsync(c.data(), d_counts, sizeof(orbgpu::MapCounts) * (size_t)count, hipMemcpyDeviceToHost, s) !=
            hipSuccess)
            return ORB_E_HIP;
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
        for (int f = 0; f < count; f++) {
            orb_localupdate& u = U[f];
            u.n_kf = c[f].n_kf; u.ref_kf = c[f].ref_kf; u.n_pt = c[f].n_pt; u.reserved = 0;
            const orbgpu::MapLocalDev& d = P[f];
            auto down = [&](void* dst, const void* src, size_t bytes) {
                return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
            };
            bool ok = down(u.cur_mp, d.q.list, 4 * (size_t)u.N);   // bad points are cleared even on an empty vote
            if (u.n_kf > 0) {
                const size_t nk = (size_t)std::min(u.n_kf, u.kf_cap), np = (size_t)std::min(u.n_pt, u.pt_cap);
                ok = ok && down(u.local_kf, d.local_kf, 4 * nk) && down(u.local_mp, d.local_mp, 4 * np) &&
                     down(u.cur_row, d.cur_row, 4 * (size_t)u.N);
                if (u.row) ok = ok && down(u.row, d.local_mp, 4 * np);
            }
            if (!ok) return ORB_E_HIP;
        }
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    }
    for (int f = 0; f < count; f++)
        if (U[f].n_kf > U[f].kf_cap || U[f].n_pt > U[f].pt_cap) return ORB_E_CAPACITY;
    return ORB_OK;
}

int Map_SetKeyFrameKeys(Map_h h, int32_t id, int N, const uint8_t* octave, const float* uRight, const float* depth,
                        float thDepth) {
    if (id < 0 || N < 0 || N > orbgpu::kMapMaxRow || (N > 0 && !octave)) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->map.set_keys(id, N, octave, uRight, depth, thDepth));
}

int LocalMapping_KeyFrameCulling(Map_h h, orb_kfcull* r) {
    if (!r || r->n < 0 || r->cap_bad < 0 || r->nbad < 0) return ORB_E_INVALID;
    if (r->n > 0 && (!r->cand || !r->nMPs || !r->nRedundant || !r->verdict)) return ORB_E_INVALID;
    if ((r->cap_bad > 0 && !r->bad_mp) || (r->nbad > 0 && !r->bad)) return ORB_E_INVALID;
    {
        std::unordered_set<int32_t> seen;   // SetBadFlag runs once per keyframe
        for (int i = 0; i < r->n; i++)
            if (!seen.insert(r->cand[i]).second) return ORB_E_INVALID;
    }
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    orbgpu::MapKfCull c{r->n, r->cand, r->not_erase, r->monocular, r->bad, r->nbad, r->cap_bad,
                        r->nMPs, r->nRedundant, r->verdict, r->bad_mp, 0};
    const int e = h->map.cull_keyframes(c);
    r->n_bad = c.n_bad;
    if (e) return rc_of(e);
    if (r->apply) {   // what Map_EraseKeyFrame / Map_EraseMapPoint would do
        for (int i = 0; i < r->n; i++)
            if (r->verdict[i] == 1)
                if (int e2 = h->map.erase_keyframe(r->cand[i])) return rc_of(e2);
        for (int i = 0; i < r->n_bad; i++)
            if (int e2 = h->map.erase_point(r->bad_mp[i])) return rc_of(e2);
    }
    return ORB_OK;
}

int LocalMapping_MapPointCulling(Map_h h, orb_pointcull* r) {
    if (!r || r->n < 0 || r->nbad < 0 || (r->nbad > 0 && !r->bad)) return ORB_E_INVALID;
    if (r->n > 0 && (!r->mp || !r->first_kf || !r->found || !r->visible || !r->verdict)) return ORB_E_INVALID;
    for (int i = 0; i < r->n; i++)
        if (r->mp[i] < 0 || r->visible[i] <= 0) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    orbgpu::MapPtCull c{r->n, r->mp, r->first_kf, r->found, r->visible, r->bad, r->nbad, r->cur_kf, r->monocular,
                        r->verdict, r->observations};
    if (int e = h->map.cull_points(c)) return rc_of(e);
    if (r->apply)
        for (int i = 0; i < r->n; i++)
            if (r->verdict[i] == 2 || r->verdict[i] == 3)
                if (int e2 = h->map.erase_point(r->mp[i])) return rc_of(e2);
    return ORB_OK;
}

int Map_enable_timing(Map_h h, int on) {
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    h->map.enable_timing(on != 0);
    return ORB_OK;
}

int Map_last_timings(Map_h h, float* ms5) {
    if (!ms5) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    const int e = h->map.timings(ms5);
    return e == 0 ? ORB_OK : e == -1 ? ORB_E_INVALID : ORB_E_HIP;
}

int orbgpu_unit_set_map_initial_capacity(int slots, int cells, int points) {
    if (slots < 0 || cells < 0 || points < 0) return 1;
    g_init_slots.store(slots > 0 ? slots : kDefaultSlots);
    g_init_cells.store(cells > 0 ? cells : kDefaultCells);
    g_init_points.store(points > 0 ? points : kDefaultPoints);
    return 0;
}

int orbgpu_unit_set_map_chunk(int frames) {
    if (frames < 0) return 1;
    g_chunk.store(frames);
    return 0;
}

int orbgpu_unit_set_map_lds_slots(int slots) {
    if (slots < -1) return 1;
    g_lds_slots.store(slots);
    return 0;
}

}  // extern "C"
