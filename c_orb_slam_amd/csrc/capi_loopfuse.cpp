// capi_loopfuse.cpp -- extern "C" LoopClosing_SearchAndFuse (include/orbslam_gpu.h): the "Start Loop
// Fusion" block of LoopClosing::CorrectLoop and LoopClosing::SearchAndFuse (src/LoopClosing.cc) with
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:977-1100),
// MapPoint::Replace and ComputeDistinctiveDescriptors (src/MapPoint.cc).
// Split of the work as in capi_fuse.cpp: the device projects every (corrected keyframe, loop point)
// pair once, matches one pass at a time against the working descriptor table and recomputes the
// descriptors of the survivors (fuse.hip, localmap.hip); the host replays the mutations on a
// copy-on-write image of the handle's relation.  No projection, gate or distance is evaluated here.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <numeric>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/orbslam_gpu.h"
#include "capi_handles.hpp"
#include "fuse.hpp"
#include "fuse_host.hpp"
#include "localmap.hpp"

namespace {

using orbgpu::FuseKF;
using orbgpu::kMapMaxRow;
using orbgpu::Map;
using orbgpu::fuse_host::al;
using orbgpu::fuse_host::Bump;
using orbgpu::fuse_host::StageTimer;
using orbgpu::fuse_host::WorkRel;

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

int no_handle() { return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID; }

bool loop_frame_ok(const orb_frame* f) {   // Tcw is not read: the pose is Scw
    if (f->N < 0 || f->N > orbgpu::kMaxFrameKeys || (f->N && (!f->keysUn || !f->desc)) || !f->scaleFactors ||
        f->nlevels <= 0)
        return false;
    for (int i = 0; i < f->N; i++)
        if (f->keysUn[i].octave < 0 || f->keysUn[i].octave >= f->nlevels) return false;
    return true;
}

// cvScw = Converter::toCvMat(g2oScw): R = q.toRotationMatrix() (Eigen's formula, in double), the
// entries (float)(s * R_ij) and (float)t_i; then ORBmatcher.cc:985-990 as pose_Scw of capi_search.cpp:
// scw = sqrt(row0 . row0), Rcw = sRcw / scw, tcw = t / scw (float multiply by (float)(1 / scw)),
// Ow = -Rcw.t() * tcw (one gemm with alpha -1).
void pose_of_sim3(const double* S8, FuseKF& D) {
    const double x = S8[0], y = S8[1], z = S8[2], w = S8[3], s = S8[7];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz),
                         tyz - twx,         txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    float sR[9], t[3];
    for (int k = 0; k < 9; k++) sR[k] = (float)(s * R[k]);
    for (int k = 0; k < 3; k++) t[k] = (float)S8[4 + k];
    const double d = (double)sR[0] * sR[0] + (double)sR[1] * sR[1] + (double)sR[2] * sR[2];
    const float scw = (float)std::sqrt(d);
    const float a = (float)(1.0 / (double)scw);
    for (int k = 0; k < 9; k++) D.R[k] = sR[k] * a + 0.0f;
    for (int k = 0; k < 3; k++) D.t[k] = t[k] * a + 0.0f;
    for (int i = 0; i < 3; i++) {
        const double acc = (double)D.R[i] * D.t[0] + (double)D.R[3 + i] * D.t[1] + (double)D.R[6 + i] * D.t[2];
        D.O[i] = (float)(acc * -1.0);
    }
}

}  // namespace

extern "C" {

int LoopClosing_SearchAndFuse(ORBmatcher_h mh, Map_h h, orb_loopfuse* F) {
    // ---- checks that need no handle
    if (!F || F->nkf < 0 || (F->nkf > 0 && (!F->kf || !F->frame || !F->Scw || !F->nfused))) return ORB_E_INVALID;
    if (F->nloop < 0 || (F->nloop > 0 && !F->loop_pts) || F->nmatched < 0) return ORB_E_INVALID;
    if (F->n_kf_rows <= 0 || !F->kf_desc || F->n < 0) return ORB_E_INVALID;
    if (F->n > 0 && (!F->pos || !F->normal || !F->max_dist || !F->min_dist || !F->desc || !F->bad)) return ORB_E_INVALID;
    if (F->cap_ops < 0 || F->cap_updated < 0 || (F->cap_ops > 0 && !F->ops) || (F->cap_updated > 0 && !F->updated))
        return ORB_E_INVALID;
    if (!std::isfinite(F->th) || F->th < 0 || !std::isfinite(F->logScaleFactor) || F->logScaleFactor == 0)
        return ORB_E_INVALID;
    const int nkf = F->nkf, nloop = F->nloop;
    const size_t np = (size_t)F->n;
    for (int k = 0; k < nkf; k++) {
        if (F->kf[k] < 0 || F->kf[k] >= F->n_kf_rows || !loop_frame_ok(&F->frame[k])) return ORB_E_INVALID;
        for (int j = 0; j < 8; j++)
            if (!std::isfinite(F->Scw[8 * (size_t)k + j])) return ORB_E_INVALID;
        if (!(F->Scw[8 * (size_t)k + 7] > 0)) return ORB_E_INVALID;
    }
    // pass order: ascending keyframe id (the pointer-keyed KeyFrameAndPose map); an id named twice
    std::vector<int> order((size_t)nkf);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return F->kf[a] < F->kf[b]; });
    for (int k = 1; k < nkf; k++)
        if (F->kf[order[(size_t)k]] == F->kf[order[(size_t)k - 1]]) return ORB_E_INVALID;
    {
        std::vector<uint8_t> seen(np, 0);
        for (int i = 0; i < nloop; i++) {
            const int32_t p = F->loop_pts[i];
            if (p < 0) continue;
            if ((size_t)p >= np || seen[(size_t)p]) return ORB_E_INVALID;
            seen[(size_t)p] = 1;
        }
    }
    const bool step0 = F->matched != nullptr;
    if (step0) {
        if (F->cur_kf < 0 || F->cur_kf >= F->n_kf_rows) return ORB_E_INVALID;
        for (int i = 0; i < F->nmatched; i++) {
            const int32_t L = F->matched[i];
            if (L >= 0 && ((size_t)L >= np || F->bad[L])) return ORB_E_INVALID;
        }
    }
    if (!mh || !h) return no_handle();
    orbgpu::Matcher* m = mh->m;
    if (m->device_pointers() || m->chain().on()) return ORB_E_INVALID;
    hipStream_t s = m->stream();
    std::lock_guard<std::mutex> lk(h->mu);
    Map& map = h->map;
    // ---- checks against the handle
    if (map.n_ids() > F->n_kf_rows) return ORB_E_INVALID;
    auto row_ok = [&](int sl) {
        const int32_t* rmp = map.row_mp(sl);
        const uint8_t* robs = map.row_obs(sl);
        for (int i = 0; i < map.row_size(sl); i++)
            if (rmp[i] >= 0 && (!robs[i] || (size_t)rmp[i] >= np)) return false;
        return true;
    };
    std::vector<int> slot((size_t)nkf);   // by pass
    int maxN = 1;
    for (int k = 0; k < nkf; k++) {
        const int c = order[(size_t)k];
        const int sl = map.slot_of(F->kf[c]);
        if (sl < 0 || F->frame[c].N != map.row_size(sl) || !row_ok(sl)) return ORB_E_INVALID;
        slot[(size_t)k] = sl;
        maxN = std::max(maxN, F->frame[c].N);
    }
    int cur_slot = -1;
    if (step0) {
        cur_slot = map.slot_of(F->cur_kf);
        if (cur_slot < 0 || F->nmatched != map.row_size(cur_slot) || !row_ok(cur_slot)) return ORB_E_INVALID;
    }
    for (int sl = 0; sl < map.n_slots(); sl++)
        if (map.slot_live(sl) && map.row_size(sl) > 0 && !F->kf_desc[map.slot_id(sl)]) return ORB_E_INVALID;

    orbgpu::LoopFuseWork& LW = h->loopfuse;
    orbgpu::FuseWork& W = LW.dev;
    W.timed = false;   // a call that fails leaves no timings of an earlier one behind
    StageTimer tm{W, s, map.timing_on()};
    double replay_ms = 0;
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };

    // ---- device image.  Buffer 0 starts with everything the call uploads, laid out as the pinned
    // staging block is: the listed keyframes' keys, descriptors and scale factors, the keyframe and
    // grid structs, the loop list and the map-point table; one copy brings all of it over.
    const size_t pairs = (size_t)std::max(nkf, 1) * (size_t)std::max(nloop, 1);
    size_t need = al(sizeof(FuseKF) * (size_t)std::max(nkf, 1)) + al(sizeof(orbgpu::SearchDev) * (size_t)std::max(nkf, 1)) +
                  al(4 * (size_t)std::max(nloop, 1)) + 2 * al(12 * np + 1) + 2 * al(4 * np + 1) + al(32 * np + 1) +
                  al(16 * pairs) + al(4 * pairs) + al((size_t)std::max(nloop, 1)) + al(4 * (size_t)std::max(nloop, 1)) +
                  4096;
    for (int k = 0; k < nkf; k++) {
        const orb_frame* f = &F->frame[k];
        need += al(28 * (size_t)f->N + 1) + al(32 * (size_t)f->N + 1) + al(4 * (size_t)(orbgpu::kGridCells + 1)) +
                al(4 * (size_t)f->N + 1) + al(4 * (size_t)f->nlevels);
    }
    Bump B;
    B.base = (char*)W.get(0, need, s);
    B.cap = need;
    if (!B.base) return ORB_E_HIP;
    std::vector<FuseKF> K((size_t)nkf);
    std::vector<orbgpu::SearchDev> G((size_t)nkf);
    struct Src {
        size_t off;
        const void* p;
        size_t bytes;
    };
    std::vector<Src> srcs;
    auto staged = [&](const void* dev, const void* src, size_t bytes) {
        if (bytes) srcs.push_back(Src{(size_t)((const char*)dev - B.base), src, bytes});
    };
    bool ok = true;
    for (int k = 0; k < nkf; k++) {
        const orb_frame* f = &F->frame[order[(size_t)k]];
        FuseKF& D = K[(size_t)k];
        std::memset(&D, 0, sizeof(D));
        pose_of_sim3(F->Scw + 8 * (size_t)order[(size_t)k], D);
        D.fx = f->fx; D.fy = f->fy; D.cx = f->cx; D.cy = f->cy; D.bf = 0.f;
        D.minX = f->minX; D.maxX = f->maxX; D.minY = f->minY; D.maxY = f->maxY;
        D.gridWInv = f->gridWInv; D.gridHInv = f->gridHInv;
        D.N = f->N;
        D.nlevels = f->nlevels;
        orbgpu::orb_kp_dev* dk = B.take<orbgpu::orb_kp_dev>((size_t)f->N);
        uint8_t* dd = B.take<uint8_t>(32 * (size_t)f->N);
        float* sc = B.take<float>((size_t)f->nlevels);
        ok = ok && dk && dd && sc;
        if (!ok) return ORB_E_HIP;
        staged(dk, f->keysUn, 28 * (size_t)f->N);
        staged(dd, f->desc, 32 * (size_t)f->N);
        staged(sc, f->scaleFactors, 4 * (size_t)f->nlevels);
        D.keys = dk; D.desc = dd; D.uRight = nullptr; D.scale = sc;
    }
    FuseKF* dK = B.take<FuseKF>((size_t)nkf);
    orbgpu::SearchDev* dG = B.take<orbgpu::SearchDev>((size_t)nkf);
    int32_t* d_loop = B.take<int32_t>((size_t)nloop);
    float* d_pos = B.take<float>(3 * np);
    float* d_normal = B.take<float>(3 * np);
    float* d_maxd = B.take<float>(np);
    float* d_mind = B.take<float>(np);
    uint8_t* d_desc = B.take<uint8_t>(32 * np);
    const size_t staged_bytes = B.used;   // the end of the uploaded prefix
    for (int k = 0; k < nkf; k++) {       // the grids are built on the device
        const orb_frame* f = &F->frame[order[(size_t)k]];
        int* gs = B.take<int>((size_t)orbgpu::kGridCells + 1);
        int* gi = B.take<int>((size_t)f->N);
        if (!gs || !gi) return ORB_E_HIP;
        K[(size_t)k].gridStart = gs;
        K[(size_t)k].gridIdx = gi;
        orbgpu::SearchDev& P = G[(size_t)k];
        std::memset(&P, 0, sizeof(P));
        P.cur.N = f->N;
        P.cur.keysUn = K[(size_t)k].keys;
        P.cur.minX = f->minX; P.cur.maxX = f->maxX; P.cur.minY = f->minY; P.cur.maxY = f->maxY;
        P.cur.gridWInv = f->gridWInv; P.cur.gridHInv = f->gridHInv;
        P.gridStart = gs;
        P.gridIdx = gi;
    }
    float4* d_uvr = B.take<float4>((size_t)nkf * (size_t)nloop);
    int32_t* d_level = B.take<int32_t>((size_t)nkf * (size_t)nloop);
    uint8_t* d_skip = B.take<uint8_t>((size_t)nloop);
    int32_t* d_best = B.take<int32_t>((size_t)nloop);
    if (!dK || !dG || !d_loop || !d_pos || !d_normal || !d_maxd || !d_mind || !d_desc || !d_uvr || !d_level || !d_skip ||
        !d_best)
        return ORB_E_HIP;
    staged(dK, K.data(), sizeof(FuseKF) * K.size());
    staged(dG, G.data(), sizeof(orbgpu::SearchDev) * G.size());
    staged(d_loop, F->loop_pts, 4 * (size_t)nloop);
    staged(d_pos, F->pos, 12 * np);
    staged(d_normal, F->normal, 12 * np);
    staged(d_maxd, F->max_dist, 4 * np);
    staged(d_mind, F->min_dist, 4 * np);
    staged(d_desc, F->desc, 32 * np);
    char* stage = (char*)LW.pinned(0, staged_bytes, s);
    // block 1: a pass's skip bytes, then its best[]; the chosen rows of a recomputation come back into the
    // best[] part (a step has at most nloop, step 0 at most nmatched survivors, and best[] is consumed by then)
    const size_t n_best = (size_t)std::max(std::max(nloop, step0 ? F->nmatched : 0), 1);
    uint8_t* pin_skip = (uint8_t*)LW.pinned(1, al((size_t)std::max(nloop, 1)) + 4 * n_best, s);
    if (!stage || !pin_skip) return ORB_E_HIP;
    int32_t* pin_best = (int32_t*)(pin_skip + al((size_t)std::max(nloop, 1)));
    for (const Src& c : srcs) std::memcpy(stage + c.off, c.p, c.bytes);
    if (hipMemcpyAsync(B.base, stage, staged_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return ORB_E_HIP;
    if (nkf > 0 && m->build_grids(dG, nkf, maxN)) return ORB_E_HIP;
    orbgpu::FuseProjDev PJ;
    std::memset(&PJ, 0, sizeof(PJ));
    PJ.kf = dK; PJ.kf_of = nullptr; PJ.ntargets = nkf; PJ.npts = nloop; PJ.pts = d_loop; PJ.n_table = F->n;
    PJ.pos = d_pos; PJ.normal = d_normal; PJ.max_dist = d_maxd; PJ.min_dist = d_mind;
    PJ.logScaleFactor = F->logScaleFactor; PJ.th = F->th;
    PJ.uvr = d_uvr; PJ.level = d_level;
    tm.begin(0);
    if (orbgpu::fuse_project_sim3_launch(PJ, s)) return ORB_E_HIP;
    tm.end();

    // ---- the replay state
    WorkRel rel(map, np);
    std::vector<uint8_t> replaced(np, 0);
    auto is_bad = [&](int32_t p) { return F->bad[p] != 0 || replaced[(size_t)p] != 0; };
    std::vector<int32_t> ops, nfused((size_t)std::max(nkf, 1), 0);
    std::unordered_map<int32_t, std::pair<int32_t, int>> new_desc;   // point -> (keyframe id, index) of its new row
    std::vector<int32_t> touched;
    std::vector<std::pair<int32_t, uint32_t>> obs;
    // the survivors of a step in order of first survival, each with its observers at its last survival
    std::vector<int32_t> surv;
    std::unordered_map<int32_t, std::vector<std::pair<int32_t, uint32_t>>> surv_obs;
    // ComputeDistinctiveDescriptors at the end of Replace / after AddObservation: returns at once for a bad point
    auto survives = [&](int32_t p) {
        if (is_bad(p)) return;
        if (!surv_obs.count(p)) surv.push_back(p);
        rel.observers(p, obs);
        surv_obs[p] = obs;
    };
    auto log = [&](int32_t pass, int32_t kind, int32_t a, int32_t b, int32_t kid, int32_t idx) {
        const int32_t e[6] = {pass, kind, a, b, kid, idx};
        ops.insert(ops.end(), e, e + 6);
    };
    auto do_replace = [&](int32_t pass, int32_t a, int32_t by, int32_t kid, int32_t idx) {
        rel.replace(a, by);
        replaced[(size_t)a] = 1;
        touched.push_back(a);
        log(pass, 2, a, by, kid, idx);
        survives(by);
    };
    // the descriptors of the survivors, on the device, into the working table
    auto recompute = [&]() -> int {
        auto t0 = clk::now();
        std::vector<int32_t> start(1, 0), ids;
        std::vector<uint8_t> rows;
        for (int32_t p : surv) {
            const auto& o = surv_obs[p];
            if (o.empty()) continue;
            ids.push_back(p);
            for (const auto& kc : o) {
                const uint8_t* src = F->kf_desc[kc.first] + 32 * (size_t)(kc.second % kMapMaxRow);
                rows.insert(rows.end(), src, src + 32);
            }
            start.push_back((int32_t)(rows.size() / 32));
        }
        replay_ms += since(t0);
        const int ns = (int)ids.size();
        if (ns > 0) {
            Bump GB;
            GB.cap = al(4 * ((size_t)ns + 1)) + 2 * al(4 * (size_t)ns) + al(rows.size()) + 1024;
            GB.base = (char*)W.get(2, GB.cap, s);
            int32_t* d_start = GB.take<int32_t>((size_t)ns + 1);
            int32_t* d_ids = GB.take<int32_t>((size_t)ns);
            int32_t* d_bi = GB.take<int32_t>((size_t)ns);
            uint8_t* d_rows = GB.take<uint8_t>(rows.size());
            if (!d_start || !d_ids || !d_bi || !d_rows) return ORB_E_HIP;
            if (hipMemcpyAsync(d_start, start.data(), 4 * ((size_t)ns + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(d_ids, ids.data(), 4 * (size_t)ns, hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(d_rows, rows.data(), rows.size(), hipMemcpyHostToDevice, s) != hipSuccess)
                return ORB_E_HIP;
            orbgpu::PointUpdateDev U;
            std::memset(&U, 0, sizeof(U));
            U.npts = ns; U.obsStart = d_start; U.obsDesc = d_rows; U.best = d_bi;
            tm.begin(2);
            if (orbgpu::point_update_launch(U, s)) return ORB_E_HIP;
            if (orbgpu::fuse_take_desc_launch(ns, d_ids, d_start, d_bi, d_rows, d_desc, s)) return ORB_E_HIP;
            tm.end();
            if ((size_t)ns > n_best) return ORB_E_HIP;
            const int32_t* bi = pin_best;
            if (hipMemcpyAsync(pin_best, d_bi, 4 * (size_t)ns, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
            if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
            for (int j = 0; j < ns; j++) {
                const auto& o = surv_obs[ids[(size_t)j]];
                if (bi[(size_t)j] < 0 || bi[(size_t)j] >= (int)o.size()) return ORB_E_HIP;
                const auto& kc = o[(size_t)bi[(size_t)j]];
                new_desc[ids[(size_t)j]] = {kc.first, (int)(kc.second % kMapMaxRow)};
                touched.push_back(ids[(size_t)j]);
            }
        }
        surv.clear();
        surv_obs.clear();
        return ORB_OK;
    };

    // ---- step 0: mvpCurrentMatchedPoints into the current keyframe (LoopClosing.cc, "Start Loop Fusion")
    int n_matched_skipped = 0;
    if (step0) {
        auto t0 = clk::now();
        for (int i = 0; i < F->nmatched; i++) {
            const int32_t L = F->matched[i];
            if (L < 0) continue;
            const int32_t c = rel.mp(cur_slot, i);
            if (c >= 0) {
                if (c != L) do_replace(-1, c, L, F->cur_kf, i);
            } else if (rel.row_holds(cur_slot, L)) {
                n_matched_skipped++;
            } else {
                rel.set_cell(cur_slot, i, L, true);
                log(-1, 1, L, -1, F->cur_kf, i);
                survives(L);
            }
        }
        replay_ms += since(t0);
        if (int e = recompute()) return e;
    }

    // ---- the passes, in ascending keyframe id
    std::vector<int32_t> in_row(np, -1);   // in_row[p] == k: a slot of pass k's keyframe holds p when the pass starts
    std::vector<int32_t> repl((size_t)std::max(nloop, 1)), repl_at((size_t)std::max(nloop, 1));
    for (int k = 0; k < nkf && nloop > 0; k++) {
        const int c = order[(size_t)k], sl = slot[(size_t)k], rowN = F->frame[c].N;
        const int32_t kid = F->kf[c];
        auto t0 = clk::now();
        bool any = false;
        for (int i = 0; i < rowN; i++) {   // spAlreadyFound = pKF->GetMapPoints(), taken when the pass starts
            const int32_t p = rel.mp(sl, i);
            if (p >= 0) in_row[(size_t)p] = k;
        }
        for (int i = 0; i < nloop; i++) {
            const int32_t p = F->loop_pts[i];
            const bool sk = p < 0 || is_bad(p) || in_row[(size_t)p] == k;
            pin_skip[i] = sk;
            any = any || !sk;
        }
        replay_ms += since(t0);
        if (!any) continue;
        if (hipMemcpyAsync(d_skip, pin_skip, (size_t)nloop, hipMemcpyHostToDevice, s) != hipSuccess) return ORB_E_HIP;
        orbgpu::FuseMatchDev MD;
        std::memset(&MD, 0, sizeof(MD));
        MD.kf = dK; MD.k = k; MD.npts = nloop; MD.pts = d_loop; MD.skip = d_skip; MD.desc = d_desc;
        MD.uvr = d_uvr + (size_t)k * (size_t)nloop; MD.level = d_level + (size_t)k * (size_t)nloop; MD.best = d_best;
        tm.begin(1);
        if (orbgpu::fuse_match_sim3_launch(MD, s)) return ORB_E_HIP;
        tm.end();
        if (hipMemcpyAsync(pin_best, d_best, 4 * (size_t)nloop, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
        // the mutations in point order (ORBmatcher.cc:1078-1095), then the Replaces (LoopClosing::SearchAndFuse)
        t0 = clk::now();
        for (int i = 0; i < nloop; i++) {
            repl[(size_t)i] = -1;
            const int b = pin_best[i];
            if (pin_skip[i] || b < 0 || b >= rowN) continue;
            const int32_t p = F->loop_pts[i];
            const int32_t q = rel.mp(sl, b);
            if (q >= 0) {
                if (!is_bad(q)) {
                    repl[(size_t)i] = q;
                    repl_at[(size_t)i] = b;
                } else {
                    log(c, 3, p, q, kid, b);
                }
            } else {
                rel.set_cell(sl, b, p, true);
                log(c, 1, p, -1, kid, b);
            }
            nfused[(size_t)c]++;
        }
        for (int i = 0; i < nloop; i++)
            if (repl[(size_t)i] >= 0) do_replace(c, repl[(size_t)i], F->loop_pts[i], kid, repl_at[(size_t)i]);
        replay_ms += since(t0);
        if (int e = recompute()) return e;
    }
    if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;   // a call without a pass has not waited yet
    tm.finish(replay_ms);

    // ---- outputs
    std::sort(touched.begin(), touched.end());
    touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    F->n_ops = (int32_t)(ops.size() / 6);
    F->n_updated = (int32_t)touched.size();
    F->n_matched_skipped = n_matched_skipped;
    if (F->n_ops > F->cap_ops || F->n_updated > F->cap_updated) return ORB_E_CAPACITY;
    if (F->apply) {   // what Map_SetMapPointMatches / Map_ReplaceMapPoint would do, in execution order
        // Neither can fail here: every op was carried out on the WorkRel image of this same handle under
        // the lock (the keyframe is live, the slot inside its row, the added point in no slot of the row),
        // and both change the host mirror only.  The error return is a guard, not a path with a rollback.
        const uint8_t one = 1;
        for (size_t k = 0; k < ops.size(); k += 6) {
            int e = 0;
            if (ops[k + 1] == 1) e = map.set_matches(ops[k + 4], 1, &ops[k + 5], &ops[k + 2], &one);
            else if (ops[k + 1] == 2) e = map.replace_point(ops[k + 2], ops[k + 3]);
            if (e) return e == -1 ? ORB_E_INVALID : ORB_E_HIP;
        }
    }
    if (nkf > 0) std::memcpy(F->nfused, nfused.data(), 4 * (size_t)nkf);
    if (!ops.empty()) std::memcpy(F->ops, ops.data(), 4 * ops.size());
    if (!touched.empty()) std::memcpy(F->updated, touched.data(), 4 * touched.size());
    for (const auto& nd : new_desc)
        std::memcpy(F->desc + 32 * (size_t)nd.first, F->kf_desc[nd.second.first] + 32 * (size_t)nd.second.second, 32);
    for (size_t p = 0; p < np; p++)
        if (replaced[p]) F->bad[p] = 1;
    return ORB_OK;
}

int LoopClosing_SearchAndFuse_last_timings(Map_h h, float* ms4) {
    if (!ms4) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    const orbgpu::FuseWork& W = h->loopfuse.dev;
    if (!W.timed) return ORB_E_INVALID;
    ms4[0] = W.ms[0];   // projection
    ms4[1] = W.ms[1];   // match
    ms4[2] = W.ms[2];   // descriptor recomputation
    ms4[3] = W.ms[4];   // the host replay
    return ORB_OK;
}

}  // extern "C"
