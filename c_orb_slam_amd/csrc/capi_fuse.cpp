// capi_fuse.cpp -- extern "C" LocalMapping_SearchInNeighbors (include/orbslam_gpu.h), reference
// src/LocalMapping.cc:454-553 with ORBmatcher::Fuse (src/ORBmatcher.cc:825-975), MapPoint::Replace,
// ComputeDistinctiveDescriptors and UpdateNormalAndDepth (src/MapPoint.cc).
// Split of the work: the device projects every (target, point) pair once, matches one pass at a
// time against the working descriptor table and recomputes the descriptors of the points a pass
// merged (fuse.hip, localmap.hip); the host keeps a copy-on-write image of the handle's relation,
// replays the pass's mutations on it in point order from one small download, and gathers the
// observer rows the recomputation needs.  No projection, gate or distance is evaluated here.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
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
using orbgpu::fuse_host::WorkRel;   // the copy-on-write relation, shared with capi_loopfuse.cpp

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

int no_handle() { return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID; }

bool fuse_frame_ok(const orb_frame* f) {
    if (!f || f->N < 0 || f->N > orbgpu::kMaxFrameKeys || (f->N && (!f->keysUn || !f->desc)) || !f->scaleFactors ||
        f->nlevels <= 0 || !f->Tcw)
        return false;
    for (int i = 0; i < f->N; i++)
        if (f->keysUn[i].octave < 0 || f->keysUn[i].octave >= f->nlevels) return false;
    return true;
}

}  // namespace

extern "C" {

int LocalMapping_SearchInNeighbors(ORBmatcher_h mh, Map_h h, orb_searchneigh* S) {
    // ---- checks that need no handle
    if (!S || !fuse_frame_ok(S->cur) || S->ntargets < 0 || (S->ntargets > 0 && (!S->target_id || !S->target)))
        return ORB_E_INVALID;
    if (S->n_kf_rows <= 0 || !S->kf_desc || !S->Ow || S->nlevels <= 0 || !S->scale_factors || S->n < 0 || !S->nfused)
        return ORB_E_INVALID;
    if (S->n > 0 && (!S->pos || !S->desc || !S->normal || !S->max_dist || !S->min_dist || !S->bad || !S->ref_kf))
        return ORB_E_INVALID;
    if (S->cap_ops < 0 || S->cap_updated < 0 || (S->cap_ops > 0 && !S->ops) || (S->cap_updated > 0 && !S->updated))
        return ORB_E_INVALID;
    if (!std::isfinite(S->th) || S->th < 0 || !std::isfinite(S->logScaleFactor) || S->logScaleFactor == 0)
        return ORB_E_INVALID;
    if (S->cur_kf < 0 || S->cur_kf >= S->n_kf_rows) return ORB_E_INVALID;
    const int nt = S->ntargets;
    for (int t = 0; t < nt; t++) {
        const int32_t id = S->target_id[t];
        if (id < 0 || id >= S->n_kf_rows || id == S->cur_kf || !fuse_frame_ok(&S->target[t])) return ORB_E_INVALID;
    }
    if (!mh || !h) return no_handle();
    orbgpu::Matcher* m = mh->m;
    if (m->device_pointers() || m->chain().on()) return ORB_E_INVALID;
    hipStream_t s = m->stream();
    std::lock_guard<std::mutex> lk(h->mu);
    Map& map = h->map;
    // ---- checks against the handle
    if (map.n_ids() > S->n_kf_rows) return ORB_E_INVALID;
    // keyframes on the device: the distinct targets in order of appearance, then cur
    std::vector<int32_t> kf_of((size_t)nt);
    std::vector<const orb_frame*> frames;
    std::vector<int32_t> frame_id;
    std::vector<int> frame_slot;
    {
        std::unordered_map<int32_t, int> seen;
        for (int t = 0; t < nt; t++) {
            auto it = seen.find(S->target_id[t]);
            if (it == seen.end()) {
                it = seen.emplace(S->target_id[t], (int)frames.size()).first;
                frames.push_back(&S->target[t]);
                frame_id.push_back(S->target_id[t]);
            } else if (S->target[t].N != frames[(size_t)it->second]->N) {
                return ORB_E_INVALID;
            }
            kf_of[(size_t)t] = it->second;
        }
        frames.push_back(S->cur);
        frame_id.push_back(S->cur_kf);
    }
    const int nu = (int)frames.size() - 1;   // index of cur
    int maxN = 1;
    for (size_t k = 0; k < frames.size(); k++) {
        const int sl = map.slot_of(frame_id[k]);
        if (sl < 0 || frames[k]->N != map.row_size(sl)) return ORB_E_INVALID;
        const int32_t* rmp = map.row_mp(sl);
        const uint8_t* robs = map.row_obs(sl);
        for (int i = 0; i < frames[k]->N; i++)
            if (rmp[i] >= 0 && (!robs[i] || rmp[i] >= S->n)) return ORB_E_INVALID;
        frame_slot.push_back(sl);
        maxN = std::max(maxN, frames[k]->N);
    }
    for (int sl = 0; sl < map.n_slots(); sl++)
        if (map.slot_live(sl) && map.row_size(sl) > 0 && !S->kf_desc[map.slot_id(sl)]) return ORB_E_INVALID;

    orbgpu::FuseWork& W = h->fuse;
    StageTimer tm{W, s, map.timing_on()};
    double replay_ms = 0;
    const size_t np = (size_t)S->n;
    const int ncur = S->cur->N;
    const int cur_slot = frame_slot[(size_t)nu];

    // ---- device image: keyframes, grids, the table, the forward projection
    size_t need = al(sizeof(FuseKF) * frames.size()) + al(sizeof(orbgpu::SearchDev) * frames.size()) +
                  al(4 * (size_t)std::max(nt, 1)) + al(4 * (size_t)std::max(ncur, 1)) + 2 * al(12 * np + 1) +
                  2 * al(4 * np + 1) + al(32 * np + 1) + al(16 * (size_t)std::max(nt, 1) * (size_t)std::max(ncur, 1)) +
                  al(4 * (size_t)std::max(nt, 1) * (size_t)std::max(ncur, 1)) + al((size_t)std::max(ncur, 1)) +
                  al(4 * (size_t)std::max(ncur, 1)) + 4096;
    for (const orb_frame* f : frames)
        need += al(28 * (size_t)f->N + 1) + al(32 * (size_t)f->N + 1) + al(4 * (size_t)f->N + 1) +
                al(4 * (size_t)(orbgpu::kGridCells + 1)) + al(4 * (size_t)f->N + 1) + al(4 * (size_t)f->nlevels);
    Bump B;
    B.base = (char*)W.get(0, need, s);
    B.cap = need;
    if (!B.base) return ORB_E_HIP;
    auto up = [&](void* d, const void* src, size_t bytes) {
        return bytes == 0 || (d && hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess);
    };
    std::vector<FuseKF> K(frames.size());
    std::vector<orbgpu::SearchDev> G(frames.size());
    bool ok = true;
    for (size_t k = 0; k < frames.size(); k++) {
        const orb_frame* f = frames[k];
        FuseKF& D = K[k];
        std::memset(&D, 0, sizeof(D));
        const float* T = f->Tcw;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) D.R[r * 3 + c] = T[r * 4 + c];
            D.t[r] = T[r * 4 + 3];
        }
        for (int i = 0; i < 3; i++) {   // Ow = -Rcw.t() * tcw: one gemm with alpha -1
            const double acc = (double)D.R[i] * D.t[0] + (double)D.R[3 + i] * D.t[1] + (double)D.R[6 + i] * D.t[2];
            D.O[i] = (float)(acc * -1.0);
        }
        D.fx = f->fx; D.fy = f->fy; D.cx = f->cx; D.cy = f->cy; D.bf = f->bf;
        D.minX = f->minX; D.maxX = f->maxX; D.minY = f->minY; D.maxY = f->maxY;
        D.gridWInv = f->gridWInv; D.gridHInv = f->gridHInv;
        D.N = f->N;
        D.nlevels = f->nlevels;
        orbgpu::orb_kp_dev* dk = B.take<orbgpu::orb_kp_dev>((size_t)f->N);
        uint8_t* dd = B.take<uint8_t>(32 * (size_t)f->N);
        float* du = f->uRight ? B.take<float>((size_t)f->N) : nullptr;
        int* gs = B.take<int>((size_t)orbgpu::kGridCells + 1);
        int* gi = B.take<int>((size_t)f->N);
        float* sc = B.take<float>((size_t)f->nlevels);
        ok = ok && dk && dd && gs && gi && sc && (!f->uRight || du);
        ok = ok && up(dk, f->keysUn, 28 * (size_t)f->N) && up(dd, f->desc, 32 * (size_t)f->N) &&
             up(du, f->uRight, f->uRight ? 4 * (size_t)f->N : 0) && up(sc, f->scaleFactors, 4 * (size_t)f->nlevels);
        D.keys = dk; D.desc = dd; D.uRight = du; D.gridStart = gs; D.gridIdx = gi; D.scale = sc;
        orbgpu::SearchDev& P = G[k];
        std::memset(&P, 0, sizeof(P));
        P.cur.N = f->N;
        P.cur.keysUn = dk;
        P.cur.minX = f->minX; P.cur.maxX = f->maxX; P.cur.minY = f->minY; P.cur.maxY = f->maxY;
        P.cur.gridWInv = f->gridWInv; P.cur.gridHInv = f->gridHInv;
        P.gridStart = gs;
        P.gridIdx = gi;
    }
    FuseKF* dK = B.take<FuseKF>(frames.size());
    orbgpu::SearchDev* dG = B.take<orbgpu::SearchDev>(frames.size());
    int32_t* d_kf_of = B.take<int32_t>((size_t)nt);
    int32_t* d_cur = B.take<int32_t>((size_t)ncur);
    float* d_pos = B.take<float>(3 * np);
    float* d_normal = B.take<float>(3 * np);
    float* d_maxd = B.take<float>(np);
    float* d_mind = B.take<float>(np);
    uint8_t* d_desc = B.take<uint8_t>(32 * np);
    float4* d_uvr = B.take<float4>((size_t)nt * (size_t)ncur);
    int32_t* d_level = B.take<int32_t>((size_t)nt * (size_t)ncur);
    uint8_t* d_skip = B.take<uint8_t>((size_t)ncur);
    int32_t* d_best = B.take<int32_t>((size_t)ncur);
    if (!ok || !dK || !dG || !d_kf_of || !d_cur || !d_pos || !d_normal || !d_maxd || !d_mind || !d_desc || !d_uvr ||
        !d_level || !d_skip || !d_best)
        return ORB_E_HIP;
    // vpMapPointMatches: the current keyframe's row when the call starts
    const std::vector<int32_t> cur_list(map.row_mp(cur_slot), map.row_mp(cur_slot) + ncur);
    ok = up(dK, K.data(), sizeof(FuseKF) * K.size()) && up(dG, G.data(), sizeof(orbgpu::SearchDev) * G.size()) &&
         up(d_kf_of, kf_of.data(), 4 * (size_t)nt) && up(d_cur, cur_list.data(), 4 * (size_t)ncur) &&
         up(d_pos, S->pos, 12 * np) && up(d_normal, S->normal, 12 * np) && up(d_maxd, S->max_dist, 4 * np) &&
         up(d_mind, S->min_dist, 4 * np) && up(d_desc, S->desc, 32 * np);
    if (!ok) return ORB_E_HIP;
    if (m->build_grids(dG, (int)G.size(), maxN)) return ORB_E_HIP;
    orbgpu::FuseProjDev PJ;
    std::memset(&PJ, 0, sizeof(PJ));
    PJ.kf = dK; PJ.kf_of = d_kf_of; PJ.ntargets = nt; PJ.npts = ncur; PJ.pts = d_cur; PJ.n_table = S->n;
    PJ.pos = d_pos; PJ.normal = d_normal; PJ.max_dist = d_maxd; PJ.min_dist = d_mind;
    PJ.logScaleFactor = S->logScaleFactor; PJ.th = S->th;
    PJ.uvr = d_uvr; PJ.level = d_level;
    tm.begin(0);
    if (orbgpu::fuse_project_launch(PJ, s)) return ORB_E_HIP;
    tm.end();

    // ---- the passes
    WorkRel rel(map, np);
    std::vector<int32_t> in_row(np, -1);   // in_row[p] == pass: an observed slot of the pass's keyframe holds p
    std::vector<uint8_t> replaced(np, 0);
    auto is_bad = [&](int32_t p) { return S->bad[p] != 0 || replaced[(size_t)p] != 0; };
    std::vector<int32_t> ops, nfused((size_t)nt + 1, 0);
    // descriptor rows this call chose: point -> (keyframe id, index)
    std::unordered_map<int32_t, std::pair<int32_t, int>> new_desc;
    std::vector<int32_t> touched;   // ids with a rewritten row (sorted and made unique at the end)
    std::vector<uint8_t> skip;
    std::vector<int32_t> best;
    std::vector<std::pair<int32_t, uint32_t>> obs;
    // the survivors of a pass in order of first survival, each with its observers at its last survival
    std::vector<int32_t> surv;
    std::unordered_map<int32_t, std::vector<std::pair<int32_t, uint32_t>>> surv_obs;

    auto run_pass = [&](int pass, int k, const std::vector<int32_t>& list, const int32_t* d_list, const float4* uvr,
                        const int32_t* level, uint8_t* dskip, int32_t* dbest) -> int {
        const int n = (int)list.size();
        const int sl = frame_slot[(size_t)k];
        const int32_t kid = frame_id[(size_t)k];
        auto t0 = std::chrono::steady_clock::now();
        skip.assign((size_t)std::max(n, 1), 1);
        bool any = false;
        for (int i = 0; i < frames[(size_t)k]->N; i++) {   // MapPoint::IsInKeyFrame(pKF) of every point at once
            const int32_t p = rel.mp(sl, i);
            if (p >= 0 && rel.observed(sl, i)) in_row[(size_t)p] = pass;
        }
        for (int i = 0; i < n; i++) {
            const int32_t p = list[(size_t)i];
            if (p < 0 || is_bad(p) || in_row[(size_t)p] == pass) continue;
            skip[(size_t)i] = 0;
            any = true;
        }
        replay_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!any) return ORB_OK;
        best.assign((size_t)n, -1);
        if (!up(dskip, skip.data(), (size_t)n)) return ORB_E_HIP;
        orbgpu::FuseMatchDev MD;
        std::memset(&MD, 0, sizeof(MD));
        MD.kf = dK; MD.k = k; MD.npts = n; MD.pts = d_list; MD.skip = dskip; MD.desc = d_desc;
        MD.uvr = uvr; MD.level = level; MD.best = dbest;
        tm.begin(1);
        if (orbgpu::fuse_match_launch(MD, s)) return ORB_E_HIP;
        tm.end();
        if (hipMemcpyAsync(best.data(), dbest, 4 * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
        // the mutations in point order (ORBmatcher.cc:951-971)
        t0 = std::chrono::steady_clock::now();
        surv.clear();
        surv_obs.clear();
        const int rowN = frames[(size_t)k]->N;
        for (int i = 0; i < n; i++) {
            const int b = best[(size_t)i];
            if (skip[(size_t)i] || b < 0 || b >= rowN) continue;
            const int32_t p = list[(size_t)i];
            const int32_t q = rel.mp(sl, b);
            int kind, a = p, by = -1;
            if (q >= 0) {
                if (!is_bad(q)) {
                    kind = 2;
                    if (rel.nobs(q) > rel.nobs(p)) { a = p; by = q; }
                    else { a = q; by = p; }
                    rel.replace(a, by);
                    replaced[(size_t)a] = 1;
                    touched.push_back(a);
                    if (!surv_obs.count(by)) surv.push_back(by);
                    rel.observers(by, obs);
                    surv_obs[by] = obs;
                } else {
                    kind = 3;
                    by = q;
                }
            } else {
                kind = 1;
                rel.set_cell(sl, b, p, true);
            }
            const int32_t e[6] = {pass, kind, a, by, kid, b};
            ops.insert(ops.end(), e, e + 6);
            nfused[(size_t)pass]++;
        }
        // ComputeDistinctiveDescriptors of the survivors: gather their observers' rows
        std::vector<int32_t> start(1, 0), ids;
        std::vector<uint8_t> rows;
        for (int32_t p : surv) {
            const auto& o = surv_obs[p];
            if (o.empty()) continue;
            ids.push_back(p);
            for (const auto& kc : o) {
                const uint8_t* src = S->kf_desc[kc.first] + 32 * (size_t)(kc.second % kMapMaxRow);
                rows.insert(rows.end(), src, src + 32);
            }
            start.push_back((int32_t)(rows.size() / 32));
        }
        replay_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const int ns = (int)ids.size();
        if (ns == 0) return ORB_OK;
        Bump GB;
        GB.cap = al(4 * ((size_t)ns + 1)) + 2 * al(4 * (size_t)ns) + al(rows.size()) + 1024;
        GB.base = (char*)W.get(2, GB.cap, s);
        int32_t* d_start = GB.take<int32_t>((size_t)ns + 1);
        int32_t* d_ids = GB.take<int32_t>((size_t)ns);
        int32_t* d_bi = GB.take<int32_t>((size_t)ns);
        uint8_t* d_rows = GB.take<uint8_t>(rows.size());
        if (!d_start || !d_ids || !d_bi || !d_rows) return ORB_E_HIP;
        if (!up(d_start, start.data(), 4 * ((size_t)ns + 1)) || !up(d_ids, ids.data(), 4 * (size_t)ns) ||
            !up(d_rows, rows.data(), rows.size()))
            return ORB_E_HIP;
        orbgpu::PointUpdateDev U;
        std::memset(&U, 0, sizeof(U));
        U.npts = ns; U.obsStart = d_start; U.obsDesc = d_rows; U.best = d_bi;
        tm.begin(2);
        if (orbgpu::point_update_launch(U, s)) return ORB_E_HIP;
        if (orbgpu::fuse_take_desc_launch(ns, d_ids, d_start, d_bi, d_rows, d_desc, s)) return ORB_E_HIP;
        tm.end();
        std::vector<int32_t> bi((size_t)ns);
        if (hipMemcpyAsync(bi.data(), d_bi, 4 * (size_t)ns, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
        for (int j = 0; j < ns; j++) {
            const auto& o = surv_obs[ids[(size_t)j]];
            if (bi[(size_t)j] < 0 || bi[(size_t)j] >= (int)o.size()) return ORB_E_HIP;
            const auto& kc = o[(size_t)bi[(size_t)j]];
            new_desc[ids[(size_t)j]] = {kc.first, (int)(kc.second % kMapMaxRow)};
            touched.push_back(ids[(size_t)j]);
        }
        return ORB_OK;
    };

    for (int t = 0; t < nt; t++)
        if (int e = run_pass(t, kf_of[(size_t)t], cur_list, d_cur, d_uvr + (size_t)t * (size_t)ncur,
                             d_level + (size_t)t * (size_t)ncur, d_skip, d_best))
            return e;

    // ---- backward pass: vpFuseCandidates (LocalMapping.cc:510-532)
    std::vector<int32_t> cand;   // outlives its upload
    const int32_t cur_index = nu;
    {
        auto t0 = std::chrono::steady_clock::now();
        std::vector<uint8_t> listed(np, 0);
        for (int t = 0; t < nt; t++) {
            const int k = kf_of[(size_t)t], sl = frame_slot[(size_t)k];
            for (int i = 0; i < frames[(size_t)k]->N; i++) {
                const int32_t p = rel.mp(sl, i);
                if (p < 0 || is_bad(p) || listed[(size_t)p]) continue;
                listed[(size_t)p] = 1;
                cand.push_back(p);
            }
        }
        replay_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const size_t nc = cand.size();
        if (nc > 0) {
            Bump BB;
            BB.cap = 2 * al(4 * nc) + al(16 * nc) + al(4 * nc) + al(nc) + 1024 + al(4);
            BB.base = (char*)W.get(1, BB.cap, s);
            int32_t* d_cand = BB.take<int32_t>(nc);
            int32_t* d_one = BB.take<int32_t>(1);
            float4* b_uvr = BB.take<float4>(nc);
            int32_t* b_level = BB.take<int32_t>(nc);
            uint8_t* b_skip = BB.take<uint8_t>(nc);
            int32_t* b_best = BB.take<int32_t>(nc);
            if (!d_cand || !d_one || !b_uvr || !b_level || !b_skip || !b_best) return ORB_E_HIP;
            if (!up(d_cand, cand.data(), 4 * nc) || !up(d_one, &cur_index, 4)) return ORB_E_HIP;
            orbgpu::FuseProjDev PB = PJ;
            PB.kf_of = d_one; PB.ntargets = 1; PB.npts = (int)nc; PB.pts = d_cand; PB.uvr = b_uvr; PB.level = b_level;
            tm.begin(0);
            if (orbgpu::fuse_project_launch(PB, s)) return ORB_E_HIP;
            tm.end();
            if (int e = run_pass(nt, nu, cand, d_cand, b_uvr, b_level, b_skip, b_best)) return e;
        }
    }

    // ---- final update of the current keyframe's points (LocalMapping.cc:543-552)
    int n_ref_missing = 0;
    std::vector<int32_t> fin;              // points with observers, in slot order
    std::vector<uint8_t> fin_missing;
    std::vector<int32_t> f_start(1, 0), f_best;
    std::vector<std::pair<int32_t, int>> f_obs;   // per observation (keyframe id, index)
    std::vector<float> f_normal, f_maxd, f_mind;
    {
        auto t0 = std::chrono::steady_clock::now();
        std::vector<uint8_t> rows;
        std::vector<float> oOw, pos, rOw, rsc, rtop;
        for (int i = 0; i < ncur; i++) {
            const int32_t p = rel.mp(cur_slot, i);
            if (p < 0 || is_bad(p)) continue;
            rel.observers(p, obs);
            if (obs.empty()) continue;
            const int32_t ref = S->ref_kf[p];
            int oct = -1;
            for (const auto& kc : obs) {
                const uint8_t* src = S->kf_desc[kc.first] + 32 * (size_t)(kc.second % kMapMaxRow);
                rows.insert(rows.end(), src, src + 32);
                oOw.insert(oOw.end(), S->Ow + 3 * (size_t)kc.first, S->Ow + 3 * (size_t)kc.first + 3);
                f_obs.emplace_back(kc.first, (int)(kc.second % kMapMaxRow));
                if (kc.first == ref) oct = map.row_oct((int)(kc.second / kMapMaxRow))[kc.second % kMapMaxRow];
            }
            const bool missing = ref < 0 || oct < 0 || oct >= S->nlevels;
            fin.push_back(p);
            fin_missing.push_back(missing);
            f_start.push_back((int32_t)f_obs.size());
            pos.insert(pos.end(), S->pos + 3 * (size_t)p, S->pos + 3 * (size_t)p + 3);
            const float* ro = missing ? S->pos + 3 * (size_t)p : S->Ow + 3 * (size_t)ref;
            rOw.insert(rOw.end(), ro, ro + 3);
            rsc.push_back(missing ? 1.0f : S->scale_factors[oct]);
            rtop.push_back(S->scale_factors[S->nlevels - 1]);
            if (missing) n_ref_missing++;
        }
        replay_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const size_t nf = fin.size(), tot = f_obs.size();
        if (nf > 0) {
            Bump FB;
            FB.cap = al(4 * (nf + 1)) + al(32 * tot) + al(12 * tot) + 2 * al(12 * nf) + 2 * al(4 * nf) + 1024;
            FB.base = (char*)W.get(2, FB.cap, s);
            int32_t* d_start = FB.take<int32_t>(nf + 1);
            uint8_t* d_rows = FB.take<uint8_t>(32 * tot);
            float* d_oOw = FB.take<float>(3 * tot);
            float* d_p = FB.take<float>(3 * nf);
            float* d_rOw = FB.take<float>(3 * nf);
            float* d_rsc = FB.take<float>(nf);
            float* d_rtop = FB.take<float>(nf);
            Bump RB;
            RB.cap = al(4 * nf) + al(12 * nf) + 2 * al(4 * nf) + 1024;
            RB.base = (char*)W.get(3, RB.cap, s);
            int32_t* d_bi = RB.take<int32_t>(nf);
            float* d_n = RB.take<float>(3 * nf);
            float* d_mx = RB.take<float>(nf);
            float* d_mn = RB.take<float>(nf);
            if (!d_start || !d_rows || !d_oOw || !d_p || !d_rOw || !d_rsc || !d_rtop || !d_bi || !d_n || !d_mx || !d_mn)
                return ORB_E_HIP;
            if (!up(d_start, f_start.data(), 4 * (nf + 1)) || !up(d_rows, rows.data(), 32 * tot) ||
                !up(d_oOw, oOw.data(), 12 * tot) || !up(d_p, pos.data(), 12 * nf) || !up(d_rOw, rOw.data(), 12 * nf) ||
                !up(d_rsc, rsc.data(), 4 * nf) || !up(d_rtop, rtop.data(), 4 * nf))
                return ORB_E_HIP;
            orbgpu::PointUpdateDev U;
            std::memset(&U, 0, sizeof(U));
            U.npts = (int)nf; U.obsStart = d_start; U.obsDesc = d_rows; U.best = d_bi;
            U.pos = d_p; U.obsOw = d_oOw; U.refOw = d_rOw; U.refScale = d_rsc; U.refScaleTop = d_rtop;
            U.normal = d_n; U.maxDist = d_mx; U.minDist = d_mn;
            tm.begin(3);
            if (orbgpu::point_update_launch(U, s)) return ORB_E_HIP;
            tm.end();
            f_best.resize(nf);
            f_normal.resize(3 * nf);
            f_maxd.resize(nf);
            f_mind.resize(nf);
            if (hipMemcpyAsync(f_best.data(), d_bi, 4 * nf, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(f_normal.data(), d_n, 12 * nf, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(f_maxd.data(), d_mx, 4 * nf, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(f_mind.data(), d_mn, 4 * nf, hipMemcpyDeviceToHost, s) != hipSuccess)
                return ORB_E_HIP;
        }
        if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
        for (size_t j = 0; j < nf; j++) {
            const int k0 = f_start[j], k1 = f_start[j + 1];
            if (f_best[j] < 0 || f_best[j] >= k1 - k0) return ORB_E_HIP;
            new_desc[fin[j]] = f_obs[(size_t)(k0 + f_best[j])];
            touched.push_back(fin[j]);
        }
    }
    tm.finish(replay_ms);

    // ---- outputs
    std::sort(touched.begin(), touched.end());
    touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    S->n_ops = (int32_t)(ops.size() / 6);
    S->n_updated = (int32_t)touched.size();
    S->n_ref_missing = n_ref_missing;
    if (S->n_ops > S->cap_ops || S->n_updated > S->cap_updated) return ORB_E_CAPACITY;
    if (S->apply) {   // what Map_SetMapPointMatches / Map_ReplaceMapPoint would do, in execution order
        const uint8_t one = 1;
        for (size_t k = 0; k < ops.size(); k += 6) {
            int e = 0;
            if (ops[k + 1] == 1) e = map.set_matches(ops[k + 4], 1, &ops[k + 5], &ops[k + 2], &one);
            else if (ops[k + 1] == 2) e = map.replace_point(ops[k + 2], ops[k + 3]);
            if (e) return e == -1 ? ORB_E_INVALID : ORB_E_HIP;
        }
    }
    std::memcpy(S->nfused, nfused.data(), 4 * nfused.size());
    if (!ops.empty()) std::memcpy(S->ops, ops.data(), 4 * ops.size());
    if (!touched.empty()) std::memcpy(S->updated, touched.data(), 4 * touched.size());
    for (const auto& nd : new_desc)
        std::memcpy(S->desc + 32 * (size_t)nd.first, S->kf_desc[nd.second.first] + 32 * (size_t)nd.second.second, 32);
    for (size_t j = 0; j < fin.size(); j++) {
        if (fin_missing[j]) continue;
        const int32_t p = fin[j];
        std::memcpy(S->normal + 3 * (size_t)p, f_normal.data() + 3 * j, 12);
        S->max_dist[p] = f_maxd[j];
        S->min_dist[p] = f_mind[j];
    }
    for (size_t p = 0; p < np; p++)
        if (replaced[p]) S->bad[p] = 1;
    return ORB_OK;
}

int LocalMapping_SearchInNeighbors_last_timings(Map_h h, float* ms5) {
    if (!ms5) return ORB_E_INVALID;
    if (!h) return no_handle();
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->fuse.timed) return ORB_E_INVALID;
    std::memcpy(ms5, h->fuse.ms, sizeof(h->fuse.ms));
    return ORB_OK;
}

}  // extern "C"
