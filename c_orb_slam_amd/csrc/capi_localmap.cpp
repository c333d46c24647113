// capi_localmap.cpp -- extern "C" entry points of LocalMapping's point creation and the
// MapPoint updates (include/orbslam_gpu.h), reference:
//   LocalMapping::CreateNewMapPoints                 src/LocalMapping.cc:207-452
//   MapPoint::ComputeDistinctiveDescriptors          src/MapPoint.cc:242-307
//   MapPoint::UpdateNormalAndDepth                   src/MapPoint.cc:331-371
// Host pointers only.  Each call packs its inputs into one staging block (one H2D copy), runs
// its kernels on the matcher's stream and fetches one result block (one D2H copy); the rows
// are scattered to the caller's arrays on the host, so a rejected pair or a point without
// observations leaves its output rows untouched.
#include <cstring>
#include <vector>

#include "capi_handles.hpp"
#include "localmap.hpp"

using orbgpu::Matcher;
using orbgpu::PointUpdateDev;
using orbgpu::TriBatch;
using orbgpu::TriKF;
using orbgpu::TriPair;

namespace {

size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

// one host block, 256-byte aligned parts
struct Stage {
    std::vector<uint8_t> buf;
    size_t add(const void* src, size_t bytes) {
        const size_t off = buf.size();
        buf.resize(off + al(bytes));
        if (bytes) std::memcpy(buf.data() + off, src, bytes);
        return off;
    }
};

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

// the handle is looked at last: a call without one is malformed where a device exists, and
// has no device to run on otherwise
int handle_error(ORBmatcher_h h) {
    if (h) return h->m->device_pointers() ? ORB_E_INVALID : ORB_OK;
    return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
}

bool tri_frame_ok(const orb_frame* f, const float* depth, const float* sigma2) {
    if (!f || f->N < 0 || (f->N && !f->keysUn) || !f->scaleFactors || !f->Tcw || f->nlevels <= 0 || !sigma2)
        return false;
    return !(f->N && f->uRight && !depth);   // a stereo keyframe needs mvDepth
}

void kf_header(const orb_frame* f, const float* sigma2, Stage& tab, TriKF& K) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) K.T[r * 4 + c] = f->Tcw[r * 4 + c];
    K.fx = f->fx; K.fy = f->fy; K.cx = f->cx; K.cy = f->cy;
    K.invfx = 1.0f / f->fx;   // KeyFrame::invfx (Frame.cc:108)
    K.invfy = 1.0f / f->fy;
    K.bf = f->bf; K.b = f->b;
    K.nlevels = f->nlevels;
    K.tab = (int)(tab.buf.size() / 4);
    const size_t o = tab.buf.size();
    tab.buf.resize(o + (size_t)f->nlevels * 8);
    std::memcpy(tab.buf.data() + o, f->scaleFactors, (size_t)f->nlevels * 4);
    std::memcpy(tab.buf.data() + o + (size_t)f->nlevels * 4, sigma2, (size_t)f->nlevels * 4);
}

}  // namespace

extern "C" {

int LocalMapping_CreateNewMapPoints_batch(ORBmatcher_h h, const orb_frame* KF1, const float* depth1,
                                          const float* levelSigma2_1, float scaleFactor, int count,
                                          const orb_triangulate* nb) {
    if (count < 0 || (count && !nb) || !tri_frame_ok(KF1, depth1, levelSigma2_1)) return ORB_E_INVALID;
    size_t total = 0;
    for (int f = 0; f < count; f++) {
        const orb_triangulate& Q = nb[f];
        if (Q.npairs < 0 || !tri_frame_ok(Q.KF2, Q.depth2, Q.levelSigma2_2)) return ORB_E_INVALID;
        if (Q.npairs && (!Q.pairs || !Q.x3D || !Q.status)) return ORB_E_INVALID;
        const bool opt = Q.normal || Q.max_dist || Q.min_dist;
        if (Q.npairs && opt && (!Q.normal || !Q.max_dist || !Q.min_dist)) return ORB_E_INVALID;
        for (int i = 0; i < Q.npairs; i++) {
            const int i1 = Q.pairs[2 * i], i2 = Q.pairs[2 * i + 1];
            if (i1 < 0 || i1 >= KF1->N || i2 < 0 || i2 >= Q.KF2->N) return ORB_E_INVALID;
            const int o1 = KF1->keysUn[i1].octave, o2 = Q.KF2->keysUn[i2].octave;
            if (o1 < 0 || o1 >= KF1->nlevels || o2 < 0 || o2 >= Q.KF2->nlevels) return ORB_E_INVALID;
        }
        total += (size_t)Q.npairs;
    }
    if (total > (size_t)0x7fffffff / 48) return ORB_E_INVALID;
    if (int e = handle_error(h)) return e;
    if (total == 0) return ORB_OK;
    Matcher* m = h->m;
    hipStream_t s = m->stream();

    // staging block: keyframe headers, level tables, pair records
    std::vector<TriKF> hdr((size_t)count + 1);
    Stage tab;
    kf_header(KF1, levelSigma2_1, tab, hdr[0]);
    std::vector<TriPair> pairs(total);
    size_t k = 0;
    for (int f = 0; f < count; f++) {
        const orb_triangulate& Q = nb[f];
        kf_header(Q.KF2, Q.levelSigma2_2, tab, hdr[(size_t)f + 1]);
        const orb_frame* F2 = Q.KF2;
        for (int i = 0; i < Q.npairs; i++, k++) {
            const int i1 = Q.pairs[2 * i], i2 = Q.pairs[2 * i + 1];
            const orb_kp &a = KF1->keysUn[i1], &b = F2->keysUn[i2];
            TriPair& P = pairs[k];
            P.x1 = a.x; P.y1 = a.y; P.oct1 = a.octave;
            P.ur1 = KF1->uRight ? KF1->uRight[i1] : -1.0f;
            P.z1 = KF1->uRight ? depth1[i1] : -1.0f;
            P.x2 = b.x; P.y2 = b.y; P.oct2 = b.octave;
            P.ur2 = F2->uRight ? F2->uRight[i2] : -1.0f;
            P.z2 = F2->uRight ? Q.depth2[i2] : -1.0f;
            P.nb = f + 1;
            P.pad = 0;
        }
    }
    Stage in;
    const size_t oH = in.add(hdr.data(), hdr.size() * sizeof(TriKF));
    const size_t oT = in.add(tab.buf.data(), tab.buf.size());
    const size_t oP = in.add(pairs.data(), pairs.size() * sizeof(TriPair));
    // result block: x3D, normal, max_dist, min_dist, status
    const size_t rX = 0, rN = rX + al(total * 12), rMx = rN + al(total * 12), rMn = rMx + al(total * 4),
                 rS = rMn + al(total * 4), rEnd = rS + al(total);
    if (m->arena_reserve(in.buf.size() + rEnd + 512)) return ORB_E_HIP;
    uint8_t* din = (uint8_t*)m->arena_alloc(in.buf.size());
    uint8_t* dout = (uint8_t*)m->arena_alloc(rEnd);
    if (!din || !dout) return ORB_E_HIP;
    if (hipMemcpyAsync(din, in.buf.data(), in.buf.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ORB_E_HIP;
    TriBatch B;
    B.kf = (const TriKF*)(din + oH);
    B.tab = (const float*)(din + oT);
    B.pairs = (const TriPair*)(din + oP);
    B.npairs = (int)total;
    B.ratioFactor = 1.5f * scaleFactor;
    B.x3D = (float*)(dout + rX);
    B.normal = (float*)(dout + rN);
    B.maxDist = (float*)(dout + rMx);
    B.minDist = (float*)(dout + rMn);
    B.status = (int8_t*)(dout + rS);
    if (orbgpu::triangulate_launch(B, s)) return ORB_E_HIP;
    std::vector<uint8_t> out(rEnd);
    if (hipMemcpyAsync(out.data(), dout, rEnd, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
    if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    const float* X = (const float*)(out.data() + rX);
    const float* Nn = (const float*)(out.data() + rN);
    const float* Mx = (const float*)(out.data() + rMx);
    const float* Mn = (const float*)(out.data() + rMn);
    const int8_t* St = (const int8_t*)(out.data() + rS);
    k = 0;
    for (int f = 0; f < count; f++) {
        const orb_triangulate& Q = nb[f];
        for (int i = 0; i < Q.npairs; i++, k++) {
            Q.status[i] = St[k];
            if (St[k] <= 0) continue;
            std::memcpy(Q.x3D + 3 * (size_t)i, X + 3 * k, 12);
            if (Q.normal) {
                std::memcpy(Q.normal + 3 * (size_t)i, Nn + 3 * k, 12);
                Q.max_dist[i] = Mx[k];
                Q.min_dist[i] = Mn[k];
            }
        }
    }
    return ORB_OK;
}

int MapPoint_Update_batch(ORBmatcher_h h, const orb_pointupdate* U) {
    if (!U || U->npts < 0) return ORB_E_INVALID;
    const int n = U->npts;
    if (n && (!U->obs_start || U->obs_start[0] != 0)) return ORB_E_INVALID;
    for (int p = 0; p < n; p++)
        if (U->obs_start[p + 1] < U->obs_start[p]) return ORB_E_INVALID;
    const size_t total = n ? (size_t)U->obs_start[n] : 0;
    const bool wantD = U->obs_desc != nullptr, wantN = U->pos != nullptr;
    if (n && wantD && !U->best) return ORB_E_INVALID;
    if (n && wantN &&
        ((total && !U->obs_Ow) || !U->ref_Ow || !U->ref_scale || !U->ref_scale_top || !U->normal || !U->max_dist ||
         !U->min_dist))
        return ORB_E_INVALID;
    if (int e = handle_error(h)) return e;
    const bool runD = wantD, runN = wantN;
    if (n == 0 || (!runD && !runN)) return ORB_OK;
    Matcher* m = h->m;
    hipStream_t s = m->stream();
    Stage in;
    const size_t oS = in.add(U->obs_start, ((size_t)n + 1) * 4);
    const size_t oD = runD ? in.add(U->obs_desc, total * 32) : 0;
    size_t oP = 0, oO = 0, oR = 0, oSc = 0, oTop = 0;
    if (runN) {
        oP = in.add(U->pos, (size_t)n * 12);
        oO = in.add(U->obs_Ow, total * 12);
        oR = in.add(U->ref_Ow, (size_t)n * 12);
        oSc = in.add(U->ref_scale, (size_t)n * 4);
        oTop = in.add(U->ref_scale_top, (size_t)n * 4);
    }
    const size_t rB = 0, rN = rB + al((size_t)n * 4), rMx = rN + al((size_t)n * 12), rMn = rMx + al((size_t)n * 4),
                 rEnd = rMn + al((size_t)n * 4);
    if (m->arena_reserve(in.buf.size() + rEnd + 512)) return ORB_E_HIP;
    uint8_t* din = (uint8_t*)m->arena_alloc(in.buf.size());
    uint8_t* dout = (uint8_t*)m->arena_alloc(rEnd);
    if (!din || !dout) return ORB_E_HIP;
    if (hipMemcpyAsync(din, in.buf.data(), in.buf.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ORB_E_HIP;
    PointUpdateDev D;
    std::memset(&D, 0, sizeof(D));
    D.npts = n;
    D.obsStart = (const int*)(din + oS);
    if (runD) D.obsDesc = din + oD;
    D.best = (int*)(dout + rB);
    if (runN) {
        D.pos = (const float*)(din + oP);
        D.obsOw = (const float*)(din + oO);
        D.refOw = (const float*)(din + oR);
        D.refScale = (const float*)(din + oSc);
        D.refScaleTop = (const float*)(din + oTop);
    }
    D.normal = (float*)(dout + rN);
    D.maxDist = (float*)(dout + rMx);
    D.minDist = (float*)(dout + rMn);
    if (orbgpu::point_update_launch(D, s)) return ORB_E_HIP;
    std::vector<uint8_t> out(rEnd);
    if (hipMemcpyAsync(out.data(), dout, rEnd, hipMemcpyDeviceToHost, s) != hipSuccess) return ORB_E_HIP;
    if (orbgpu::stream_wait(s) != hipSuccess) return ORB_E_HIP;
    if (runD) std::memcpy(U->best, out.data() + rB, (size_t)n * 4);
    if (runN) {
        const float* Nn = (const float*)(out.data() + rN);
        const float* Mx = (const float*)(out.data() + rMx);
        const float* Mn = (const float*)(out.data() + rMn);
        for (int p = 0; p < n; p++) {
            if (U->obs_start[p + 1] == U->obs_start[p]) continue;
            std::memcpy(U->normal + 3 * (size_t)p, Nn + 3 * (size_t)p, 12);
            U->max_dist[p] = Mx[p];
            U->min_dist[p] = Mn[p];
        }
    }
    return ORB_OK;
}

}  // extern "C"
