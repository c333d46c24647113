// fuse.hip -- gfx950 kernels of LocalMapping::SearchInNeighbors (reference
// src/LocalMapping.cc:454-553): the part of every ORBmatcher::Fuse(pKF, vpMapPoints, th) call
// (src/ORBmatcher.cc:825-975) that does not depend on the map mutations between the calls, and
// the part that does.
//
//   k_fuse_project    one thread per (target keyframe, listed point): camera coordinates, the
//                     depth / image / distance / viewing-angle gates, PredictScale and the search
//                     radius (ORBmatcher.cc:849-905).  Positions, normals and the distance range
//                     do not change before the end of SearchInNeighbors, so one launch covers every
//                     forward pass; the backward pass (its point list is known only after them)
//                     is a second launch with one target.
//   k_fuse_match      one thread per listed point of one pass: KeyFrame::GetFeaturesInArea over the
//                     keyframe's grid in the reference's cell and index order, the level gate, the
//                     5.99 / 7.8 reprojection gate, the 256-bit Hamming distance against the point's
//                     current descriptor with strict '<' (the first candidate wins a tie), accepted
//                     at <= TH_LOW (907-949).  A window holds around ten keypoints, so a thread's
//                     loop is short; the pass is bound by its launch and the download that follows,
//                     not by arithmetic, and blocks of 64 spread the few thousand points over CUs.
//   k_fuse_take_desc  the row k_distinctive chose, copied into the working descriptor table.
//   k_fuse_project_sim3 / k_fuse_match_sim3
//                     the same two steps for LoopClosing::SearchAndFuse (LoopClosing.cc), whose passes are
//                     ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:977-1100):
//                     one projection launch over every (corrected keyframe, loop point) pair, one match
//                     launch per pass, without the reprojection gate.
//
// Float expressions keep the reference's operation order (-ffp-contract=off, correctly rounded
// f32 divide / sqrt); cv::Mat products accumulate in double and round once.  They
// are those of project_point / fuse_common in capi_search.cpp, which ORBmatcher_Fuse runs on the
// host; PredictScale's logf is detmath's restatement.
#include "detmath.hpp"
#include "fuse.hpp"
#include "orb_common.hpp"
#include "orb_match.hpp"

namespace orbgpu {

namespace {

constexpr int kFuseThLow = 50;   // ORBmatcher::TH_LOW

// row r of Rcw * X + tcw as one cv::gemm: the sum in double, the translation added in double
__device__ __forceinline__ float gemm3(const float* R, const float* t, int r, const float* X) {
    const double s = (double)R[r * 3 + 0] * X[0] + (double)R[r * 3 + 1] * X[1] + (double)R[r * 3 + 2] * X[2];
    return (float)(s + (double)t[r]);
}

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__global__ void __launch_bounds__(256) k_fuse_project(FuseProjDev P) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)P.ntargets * P.npts) return;
    const int t = (int)(g / P.npts), i = (int)(g % P.npts);
    P.level[g] = -1;
    const int p = P.pts[i];
    if (p < 0 || p >= P.n_table) return;
    const FuseKF& K = P.kf[P.kf_of[t]];
    const float X[3] = {P.pos[3 * (size_t)p], P.pos[3 * (size_t)p + 1], P.pos[3 * (size_t)p + 2]};
    const float xc = gemm3(K.R, K.t, 0, X), yc = gemm3(K.R, K.t, 1, X), zc = gemm3(K.R, K.t, 2, X);
    if (zc < 0.0f) return;
    const float invz = 1 / zc;
    const float x = xc * invz, y = yc * invz;
    const float u = K.fx * x + K.cx;
    const float v = K.fy * y + K.cy;
    if (!(u >= K.minX && u < K.maxX && v >= K.minY && v < K.maxY)) return;   // KeyFrame::IsInImage
    const float ur = u - K.bf * invz;
    const float maxD = P.max_dist[p], minD = P.min_dist[p];
    const float PO[3] = {X[0] - K.O[0], X[1] - K.O[1], X[2] - K.O[2]};
    double s2 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) s2 += (double)PO[k] * (double)PO[k];
    const float dist = (float)sqrt(s2);
    if (dist < 0.8f * minD || dist > 1.2f * maxD) return;
    const float* Pn = P.normal + 3 * (size_t)p;
    const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
    if (dot < 0.5 * dist) return;
    const int lvl = detmath::predict_scale(maxD, dist, P.logScaleFactor, K.nlevels);
    P.uvr[g] = make_float4(u, v, ur, P.th * K.scale[lvl]);
    P.level[g] = lvl;
}

__global__ void __launch_bounds__(64) k_fuse_match(FuseMatchDev M) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M.npts) return;
    int out = -1;
    const int lvl = M.level[i];
    if (!M.skip[i] && lvl >= 0) {
        const FuseKF& K = M.kf[M.k];
        const float4 q = M.uvr[i];
        const float r = q.w;
        const uint4* pd = reinterpret_cast<const uint4*>(M.desc + 32 * (size_t)M.pts[i]);
        const uint4 a0 = pd[0], a1 = pd[1];
        // KeyFrame::GetFeaturesInArea (KeyFrame.cc:569-608)
        const int nMinCellX = max(0, (int)floorf((q.x - K.minX - r) * K.gridWInv));
        const int nMaxCellX = min(kGridCols - 1, (int)ceilf((q.x - K.minX + r) * K.gridWInv));
        const int nMinCellY = max(0, (int)floorf((q.y - K.minY - r) * K.gridHInv));
        const int nMaxCellY = min(kGridRows - 1, (int)ceilf((q.y - K.minY + r) * K.gridHInv));
        int bestDist = 256, bestIdx = -1;
        if (nMinCellX < kGridCols && nMaxCellX >= 0 && nMinCellY < kGridRows && nMaxCellY >= 0)
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
                for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                    const int c = ix * kGridRows + iy;
                    const int e = K.gridStart[c + 1];
                    for (int j = K.gridStart[c]; j < e; j++) {
                        const int idx = K.gridIdx[j];
                        const orb_kp_dev kp = K.keys[idx];
                        if (!(fabsf(kp.x - q.x) < r && fabsf(kp.y - q.y) < r)) continue;
                        if (kp.octave < lvl - 1 || kp.octave > lvl) continue;
                        // the reprojection gate (914-938)
                        const float sc = K.scale[kp.octave];
                        const float invSigma2 = 1.0f / (sc * sc);
                        const float ex = q.x - kp.x, ey = q.y - kp.y;
                        const float kur = K.uRight ? K.uRight[idx] : -1.0f;
                        if (kur >= 0) {
                            const float er = q.z - kur;
                            const float e2 = ex * ex + ey * ey + er * er;
                            if (e2 * invSigma2 > 7.8) continue;
                        } else {
                            const float e2 = ex * ex + ey * ey;
                            if (e2 * invSigma2 > 5.99) continue;
                        }
                        const uint4* kd = reinterpret_cast<const uint4*>(K.desc + 32 * (size_t)idx);
                        const int d = hamming256(a0, a1, kd[0], kd[1]);
                        if (d < bestDist) {
                            bestDist = d;
                            bestIdx = idx;
                        }
                    }
                }
        if (bestDist <= kFuseThLow) out = bestIdx;
    }
    M.best[i] = out;
}

// ---- LoopClosing::SearchAndFuse: ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (ORBmatcher.cc:977-1100).  K.R / K.t / K.O hold the decomposition of Scw (Rcw = sRcw / scw, tcw =
// t / scw, Ow); the listed keyframe of pair g is kf[g / npts] (kf_of is not read).  Against
// k_fuse_project: invz = 1.0 / z in double, rounded once, and no uRight (uvr.z = 0).
__global__ void __launch_bounds__(256) k_fuse_project_sim3(FuseProjDev P) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)P.ntargets * P.npts) return;
    const int t = (int)(g / P.npts), i = (int)(g % P.npts);
    P.level[g] = -1;
    const int p = P.pts[i];
    if (p < 0 || p >= P.n_table) return;
    const FuseKF& K = P.kf[t];
    const float X[3] = {P.pos[3 * (size_t)p], P.pos[3 * (size_t)p + 1], P.pos[3 * (size_t)p + 2]};
    const float xc = gemm3(K.R, K.t, 0, X), yc = gemm3(K.R, K.t, 1, X), zc = gemm3(K.R, K.t, 2, X);
    if (zc < 0.0f) return;
    const float invz = (float)(1.0 / (double)zc);
    const float x = xc * invz, y = yc * invz;
    const float u = K.fx * x + K.cx;
    const float v = K.fy * y + K.cy;
    if (!(u >= K.minX && u < K.maxX && v >= K.minY && v < K.maxY)) return;   // KeyFrame::IsInImage
    const float maxD = P.max_dist[p], minD = P.min_dist[p];
    const float PO[3] = {X[0] - K.O[0], X[1] - K.O[1], X[2] - K.O[2]};
    double s2 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) s2 += (double)PO[k] * (double)PO[k];
    const float dist = (float)sqrt(s2);
    if (dist < 0.8f * minD || dist > 1.2f * maxD) return;
    const float* Pn = P.normal + 3 * (size_t)p;
    const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
    if (dot < 0.5 * dist) return;
    const int lvl = detmath::predict_scale(maxD, dist, P.logScaleFactor, K.nlevels);
    P.uvr[g] = make_float4(u, v, 0.0f, P.th * K.scale[lvl]);
    P.level[g] = lvl;
}

// One thread per listed point of one pass, as k_fuse_match without the reprojection gate
// (ORBmatcher.cc:1050-1076).  A point whose level is >= 0 passed k_fuse_project_sim3's check of its id
// against the table, so pts[i] indexes desc only then; the three loops are bounded by the grid
// tables (cells clamped to the grid, gridStart[c + 1] <= N).  The window walk is written out again
// rather than shared with k_fuse_match through a template with a gate functor: that kernel has to
// stay bit for bit what it is, and only the __device__ helpers gemm3 / hamming256 are shared.
__global__ void __launch_bounds__(64) k_fuse_match_sim3(FuseMatchDev M) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M.npts) return;
    int out = -1;
    const int lvl = M.level[i];
    if (!M.skip[i] && lvl >= 0) {
        const FuseKF& K = M.kf[M.k];
        const float4 q = M.uvr[i];
        const float r = q.w;
        const uint4* pd = reinterpret_cast<const uint4*>(M.desc + 32 * (size_t)M.pts[i]);
        const uint4 a0 = pd[0], a1 = pd[1];
        // KeyFrame::GetFeaturesInArea (KeyFrame.cc:569-608)
        const int nMinCellX = max(0, (int)floorf((q.x - K.minX - r) * K.gridWInv));
        const int nMaxCellX = min(kGridCols - 1, (int)ceilf((q.x - K.minX + r) * K.gridWInv));
        const int nMinCellY = max(0, (int)floorf((q.y - K.minY - r) * K.gridHInv));
        const int nMaxCellY = min(kGridRows - 1, (int)ceilf((q.y - K.minY + r) * K.gridHInv));
        int bestDist = 256, bestIdx = -1;
        if (nMinCellX < kGridCols && nMaxCellX >= 0 && nMinCellY < kGridRows && nMaxCellY >= 0)
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
                for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                    const int c = ix * kGridRows + iy;
                    const int e = min(K.gridStart[c + 1], K.N);
                    for (int j = max(K.gridStart[c], 0); j < e; j++) {
                        const int idx = K.gridIdx[j];
                        if (idx < 0 || idx >= K.N) continue;
                        const orb_kp_dev kp = K.keys[idx];
                        if (!(fabsf(kp.x - q.x) < r && fabsf(kp.y - q.y) < r)) continue;
                        if (kp.octave < lvl - 1 || kp.octave > lvl) continue;
                        const uint4* kd = reinterpret_cast<const uint4*>(K.desc + 32 * (size_t)idx);
                        const int d = hamming256(a0, a1, kd[0], kd[1]);
                        if (d < bestDist) {
                            bestDist = d;
                            bestIdx = idx;
                        }
                    }
                }
        if (bestDist <= kFuseThLow) out = bestIdx;
    }
    M.best[i] = out;
}

__global__ void __launch_bounds__(256) k_fuse_take_desc(int npts, const int32_t* id, const int32_t* start,
                                                        const int32_t* best, const uint8_t* rows, uint8_t* table) {
    const int g = blockIdx.x * 256 + threadIdx.x;   // two 16-byte halves per point
    const int p = g >> 1;
    if (p >= npts) return;
    const int b = best[p];
    if (b < 0) return;
    const uint4* src = reinterpret_cast<const uint4*>(rows + 32 * (size_t)(start[p] + b));
    uint4* dst = reinterpret_cast<uint4*>(table + 32 * (size_t)id[p]);
    dst[g & 1] = src[g & 1];
}

}  // namespace

FuseWork::~FuseWork() {
    for (void* b : buf)
        if (b) (void)hipFree(b);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

void* FuseWork::get(int i, size_t bytes, hipStream_t s) {
    if (bytes <= cap[i] && buf[i]) return buf[i];
    if (buf[i]) {
        if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
        (void)hipFree(buf[i]);
        buf[i] = nullptr;
        cap[i] = 0;
    }
    const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 16);
    if (hipMalloc(&buf[i], want) != hipSuccess) {
        buf[i] = nullptr;
        return nullptr;
    }
    cap[i] = want;
    return buf[i];
}

hipEvent_t FuseWork::event(size_t k) {
    while (ev.size() <= k) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ev.push_back(e);
    }
    return ev[k];
}

int fuse_project_launch(const FuseProjDev& P, hipStream_t s) {
    const long long n = (long long)P.ntargets * P.npts;
    if (n <= 0) return 0;
    if (n > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(k_fuse_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

int fuse_match_launch(const FuseMatchDev& M, hipStream_t s) {
    if (M.npts <= 0) return 0;
    hipLaunchKernelGGL(k_fuse_match, dim3((unsigned)((M.npts + 63) / 64)), dim3(64), 0, s, M);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

int fuse_project_sim3_launch(const FuseProjDev& P, hipStream_t s) {
    const long long n = (long long)P.ntargets * P.npts;
    if (n <= 0) return 0;
    if (n > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(k_fuse_project_sim3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

int fuse_match_sim3_launch(const FuseMatchDev& M, hipStream_t s) {
    if (M.npts <= 0) return 0;
    hipLaunchKernelGGL(k_fuse_match_sim3, dim3((unsigned)((M.npts + 63) / 64)), dim3(64), 0, s, M);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

LoopFuseWork::~LoopFuseWork() {
    for (void* p : pin)
        if (p) (void)hipHostFree(p);
}

void* LoopFuseWork::pinned(int i, size_t bytes, hipStream_t s) {
    if (bytes <= pin_cap[i] && pin[i]) return pin[i];
    if (pin[i]) {
        if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
        (void)hipHostFree(pin[i]);
        pin[i] = nullptr;
        pin_cap[i] = 0;
    }
    const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 16);
    if (hipHostMalloc(&pin[i], want) != hipSuccess) {
        pin[i] = nullptr;
        return nullptr;
    }
    pin_cap[i] = want;
    return pin[i];
}

int fuse_take_desc_launch(int npts, const int32_t* id, const int32_t* start, const int32_t* best,
                          const uint8_t* rows, uint8_t* table, hipStream_t s) {
    if (npts <= 0) return 0;
    hipLaunchKernelGGL(k_fuse_take_desc, dim3((unsigned)((2 * npts + 255) / 256)), dim3(256), 0, s, npts, id, start, best,
                       rows, table);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace orbgpu
