// localmap.hip -- gfx950 kernels for LocalMapping's per-keyframe numeric work that is not a
// search or an optimisation:
//   k_triangulate   LocalMapping::CreateNewMapPoints, the geometry applied to every pair that
//                   SearchForTriangulation returns (LocalMapping.cc:262-437), one thread per pair
//                   over the concatenated pair lists of all neighbours: one launch per call.
//   k_distinctive   MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307), one workgroup per point.
//   k_normal_depth  MapPoint::UpdateNormalAndDepth (MapPoint.cc:331-371), one thread per point.
// Float expressions follow the reference's operation order (the build has -ffp-contract=off and
// correctly rounded f32 div/sqrt); every small cv::Mat product, Mat::dot and cv::norm accumulates
// in double and rounds once, as everywhere in this library.
#include <cfloat>

#include "detmath.hpp"
#include "localmap.hpp"
#include "orb_common.hpp"
#include "stereo.hpp"
#include "svd4.hpp"

namespace orbgpu {

namespace {

struct KFPose {
    float Twc[12];   // [Rwc | Ow]
};

// Rwc = Rcw^T, Ow = -Rwc * tcw (one gemm with alpha -1: f64 accumulation, one rounding)
__device__ __forceinline__ void kf_pose(const float (&T)[12], KFPose& P) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) P.Twc[r * 4 + c] = T[c * 4 + r];
        const double s = ((double)T[0 * 4 + r] * T[3] + (double)T[1 * 4 + r] * T[7]) + (double)T[2 * 4 + r] * T[11];
        P.Twc[r * 4 + 3] = (float)(s * -1.0);
    }
}

// row r of Rcw * X + tcw: Mat::dot in double, the float translation added in double
__device__ __forceinline__ float cam_row(const float (&T)[12], int r, const float (&X)[3]) {
    const double d = ((double)T[r * 4 + 0] * X[0] + (double)T[r * 4 + 1] * X[1]) + (double)T[r * 4 + 2] * X[2];
    return (float)(d + (double)T[r * 4 + 3]);
}

__device__ __forceinline__ double norm3_d(const float (&v)[3]) {
    return sqrt(((double)v[0] * v[0] + (double)v[1] * v[1]) + (double)v[2] * v[2]);
}

// cos(2 * atan2(mb / 2, depth)) on float inputs, evaluated in double, rounded once
__device__ __forceinline__ float cos_parallax_stereo(float b, float depth) {
    const double a = detmath::atan2_d((double)(b / 2), (double)depth);
    double s, c;
    detmath::sincos_d(2.0 * a, &s, &c);
    return (float)c;
}

// the reprojection test of one keyframe; true = rejected
__device__ __forceinline__ bool reproj_fails(const TriKF& K, const float (&T)[12], const float (&X)[3], float z,
                                             float kx, float ky, float kur, bool stereo, float sigma2) {
    const float x = cam_row(T, 0, X), y = cam_row(T, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = K.fx * x * invz + K.cx;
    const float v = K.fy * y * invz + K.cy;
    const float ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float ur = u - K.bf * invz;
    const float er = ur - kur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

__device__ __forceinline__ void load_T(const TriKF& K, float (&T)[12]) {
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = K.T[k];
}

}  // namespace

__global__ void __launch_bounds__(64) k_triangulate(TriBatch B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.npairs) return;
    const TriPair pr = B.pairs[i];
    const TriKF& K1 = B.kf[0];
    const TriKF& K2 = B.kf[pr.nb];
    float T1[12], T2[12];
    load_T(K1, T1);
    load_T(K2, T2);
    KFPose P1, P2;
    kf_pose(T1, P1);
    kf_pose(T2, P2);

    // parallax between the rays
    const float xn1[3] = {(pr.x1 - K1.cx) * K1.invfx, (pr.y1 - K1.cy) * K1.invfy, 1.0f};
    const float xn2[3] = {(pr.x2 - K2.cx) * K2.invfx, (pr.y2 - K2.cy) * K2.invfy, 1.0f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ray1[r] = (float)(((double)P1.Twc[r * 4 + 0] * xn1[0] + (double)P1.Twc[r * 4 + 1] * xn1[1]) +
                          (double)P1.Twc[r * 4 + 2] * xn1[2]);
        ray2[r] = (float)(((double)P2.Twc[r * 4 + 0] * xn2[0] + (double)P2.Twc[r * 4 + 1] * xn2[1]) +
                          (double)P2.Twc[r * 4 + 2] * xn2[2]);
    }
    const double dot = ((double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1]) + (double)ray1[2] * ray2[2];
    const float cosParallaxRays = (float)(dot / (norm3_d(ray1) * norm3_d(ray2)));

    const bool bStereo1 = pr.ur1 >= 0, bStereo2 = pr.ur2 >= 0;
    float cosParallaxStereo1 = cosParallaxRays + 1;
    float cosParallaxStereo2 = cosParallaxStereo1;
    if (bStereo1) cosParallaxStereo1 = cos_parallax_stereo(K1.b, pr.z1);
    else if (bStereo2) cosParallaxStereo2 = cos_parallax_stereo(K2.b, pr.z2);
    const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;

    float X[3];
    int8_t st;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
        (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        // linear triangulation; At = A^T
        float At[4][4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            At[k][0] = xn1[0] * T1[8 + k] - T1[k];
            At[k][1] = xn1[1] * T1[8 + k] - T1[4 + k];
            At[k][2] = xn2[0] * T2[8 + k] - T2[k];
            At[k][3] = xn2[1] * T2[8 + k] - T2[4 + k];
        }
        float h[4];
        svd4_vt3(At, h);
        if (h[3] == 0) {
            B.status[i] = -1;
            return;
        }
        const float inv = (float)(1.0 / (double)h[3]);
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = h[r] * inv;
        st = 1;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        unproject_point(P1.Twc, pr.x1, pr.y1, pr.z1, K1.cx, K1.cy, K1.invfx, K1.invfy, X);
        st = 2;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        unproject_point(P2.Twc, pr.x2, pr.y2, pr.z2, K2.cx, K2.cy, K2.invfx, K2.invfy, X);
        st = 3;
    } else {
        B.status[i] = 0;
        return;
    }

    // positive depth in both cameras, then the reprojection tests
    const float z1 = cam_row(T1, 2, X);
    if (z1 <= 0) {
        B.status[i] = -2;
        return;
    }
    const float z2 = cam_row(T2, 2, X);
    if (z2 <= 0) {
        B.status[i] = -4;
        return;
    }
    const float* tab1 = B.tab + K1.tab;
    const float* tab2 = B.tab + K2.tab;
    if (reproj_fails(K1, T1, X, z1, pr.x1, pr.y1, pr.ur1, bStereo1, tab1[K1.nlevels + pr.oct1])) {
        B.status[i] = -3;
        return;
    }
    if (reproj_fails(K2, T2, X, z2, pr.x2, pr.y2, pr.ur2, bStereo2, tab2[K2.nlevels + pr.oct2])) {
        B.status[i] = -5;
        return;
    }

    // scale consistency
    const float n1[3] = {X[0] - P1.Twc[3], X[1] - P1.Twc[7], X[2] - P1.Twc[11]};
    const float n2[3] = {X[0] - P2.Twc[3], X[1] - P2.Twc[7], X[2] - P2.Twc[11]};
    const double nd1 = norm3_d(n1), nd2 = norm3_d(n2);
    const float dist1 = (float)nd1, dist2 = (float)nd2;
    if (dist1 == 0 || dist2 == 0) {
        B.status[i] = -6;
        return;
    }
    const float ratioDist = dist2 / dist1;
    const float sf1 = tab1[pr.oct1];
    const float ratioOctave = sf1 / tab2[pr.oct2];
    if (ratioDist * B.ratioFactor < ratioOctave || ratioDist > ratioOctave * B.ratioFactor) {
        B.status[i] = -7;
        return;
    }

    B.status[i] = st;
#pragma unroll
    for (int r = 0; r < 3; r++) B.x3D[3 * i + r] = X[r];
    // the new point's UpdateNormalAndDepth: observations {KF1, KF2}, reference keyframe KF1
    const float i1 = (float)(1.0 / nd1), i2 = (float)(1.0 / nd2);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float acc = 0.0f;
        acc = acc + n1[r] * i1;
        acc = acc + n2[r] * i2;
        B.normal[3 * i + r] = acc * 0.5f;
    }
    const float mx = dist1 * sf1;
    B.maxDist[i] = mx;
    B.minDist[i] = mx / tab1[K1.nlevels - 1];
}

int triangulate_launch(const TriBatch& B, hipStream_t s) {
    if (B.npairs <= 0) return 0;
    hipLaunchKernelGGL(k_triangulate, dim3((B.npairs + 63) / 64), dim3(64), 0, s, B);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------- MapPoint::ComputeDistinctiveDescriptors
// One workgroup of four waves per point, one lane per row (k <= 64, the common case, is one
// wave; the other waves only help staging).  Row i's median of D[i][.] (self distance included)
// is the floor(0.5 * (k - 1))-th order statistic: the smallest v with #{j : D[i][j] <= v} >= m + 1.
// Distances lie in 0..256, so a counting select finds it without a per-lane distance array, in
// two passes over the row: 16 counters for the thresholds 15, 31, .., 255 pick the bucket of 16
// values, 16 counters for base .. base + 15 pick the value (256 itself when no bucket reaches
// the count).  The counters have static indices and stay in registers.  The first kDescLds
// descriptors of the point sit in LDS (every lane reads the same row: a broadcast), the rest
// are read from global memory.  Lanes stride over the rows; a min-reduction (wave shuffles, then
// one LDS word per wave) on (median << 32 | i) picks the smallest median, the first row on a tie (the reference's strict
// '<' against INT_MAX).
constexpr int kDescLds = 512;       // descriptors staged per point: 16 KiB
constexpr int kDescThreads = 256;   // four waves per point: rows beyond the first 64 go to the other SIMDs

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// smallest c in 0..15 with #{j : D[i][j] <= first + step * c} >= need, 16 if none
__device__ __forceinline__ int count_select16(const uint4& a0, const uint4& a1, const uint4* sd, const uint4* g, int kl,
                                              int k, int first, int step, int need) {
    int cnt[16];
#pragma unroll
    for (int c = 0; c < 16; c++) cnt[c] = 0;
#pragma unroll 2
    for (int j = 0; j < kl; j++) {
        const int d = hamming256(a0, a1, sd[2 * j], sd[2 * j + 1]) - first;
#pragma unroll
        for (int c = 0; c < 16; c++) cnt[c] += d <= step * c ? 1 : 0;
    }
    for (int j = kl; j < k; j++) {
        const int d = hamming256(a0, a1, g[2 * (size_t)j], g[2 * (size_t)j + 1]) - first;
#pragma unroll
        for (int c = 0; c < 16; c++) cnt[c] += d <= step * c ? 1 : 0;
    }
    int sel = 16;
#pragma unroll
    for (int c = 15; c >= 0; c--) sel = cnt[c] >= need ? c : sel;
    return sel;
}

__global__ void __launch_bounds__(kDescThreads) k_distinctive(PointUpdateDev U) {
    __shared__ uint4 sd[kDescLds * 2];
    __shared__ unsigned long long red[kDescThreads / 64];
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const int o0 = U.obsStart[p];
    const int k = U.obsStart[p + 1] - o0;
    if (k <= 0) {
        if (tid == 0) U.best[p] = -1;
        return;
    }
    const uint4* g = (const uint4*)U.obsDesc + 2 * (size_t)o0;
    const int kl = k < kDescLds ? k : kDescLds;
    for (int t = tid; t < 2 * kl; t += kDescThreads) sd[t] = g[t];
    __syncthreads();
    const int need = (k - 1) / 2 + 1;   // m + 1, m = (int)(0.5 * (k - 1))
    unsigned long long key = ~0ull;
    for (int i = tid; i < k; i += kDescThreads) {
        const uint4 a0 = i < kl ? sd[2 * i] : g[2 * (size_t)i];
        const uint4 a1 = i < kl ? sd[2 * i + 1] : g[2 * (size_t)i + 1];
        int median = 256;
        const int bucket = count_select16(a0, a1, sd, g, kl, k, 15, 16, need);
        if (bucket < 16) median = 16 * bucket + count_select16(a0, a1, sd, g, kl, k, 16 * bucket, 1, need);
        const unsigned long long kk = ((unsigned long long)median << 32) | (unsigned)i;
        key = kk < key ? kk : key;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other < key ? other : key;
    }
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kDescThreads / 64; w++) key = red[w] < key ? red[w] : key;
        U.best[p] = (int)(unsigned)key;
    }
}

// ------------------------------------------------------- MapPoint::UpdateNormalAndDepth
// One thread per point; the sum over the observations runs in the given order (float addition
// order is part of the semantics).  normali / cv::norm(normali): the norm in double, the
// vector scaled by (float)(1 / norm); normal / n likewise.
__global__ void __launch_bounds__(256) k_normal_depth(PointUpdateDev U) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= U.npts) return;
    const int o0 = U.obsStart[p], o1 = U.obsStart[p + 1];
    if (o1 <= o0) return;
    const float X[3] = {U.pos[3 * p], U.pos[3 * p + 1], U.pos[3 * p + 2]};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int o = o0; o < o1; o++) {
        const float* O = U.obsOw + 3 * (size_t)o;
        const float v[3] = {X[0] - O[0], X[1] - O[1], X[2] - O[2]};
        const float inv = (float)(1.0 / norm3_d(v));
#pragma unroll
        for (int r = 0; r < 3; r++) acc[r] = acc[r] + v[r] * inv;
    }
    const float invn = (float)(1.0 / (double)(o1 - o0));
#pragma unroll
    for (int r = 0; r < 3; r++) U.normal[3 * p + r] = acc[r] * invn;
    const float PC[3] = {X[0] - U.refOw[3 * p], X[1] - U.refOw[3 * p + 1], X[2] - U.refOw[3 * p + 2]};
    const float dist = (float)norm3_d(PC);
    const float mx = dist * U.refScale[p];
    U.maxDist[p] = mx;
    U.minDist[p] = mx / U.refScaleTop[p];
}

int point_update_launch(const PointUpdateDev& U, hipStream_t s) {
    if (U.npts <= 0) return 0;
    if (U.obsDesc) hipLaunchKernelGGL(k_distinctive, dim3(U.npts), dim3(kDescThreads), 0, s, U);
    if (U.pos) hipLaunchKernelGGL(k_normal_depth, dim3((U.npts + 255) / 256), dim3(256), 0, s, U);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace orbgpu
