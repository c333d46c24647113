// initializer.hpp -- ORB_SLAM2::Initializer (src/Initializer.cc) on the GPU: the device layout of
// one Initialize call and the small CV_32F matrix operations host and device share.
//
// OpenCV semantics of a small float matrix: a product accumulates each element in double in k
// order and rounds once (gemm, alpha applied in double); the 3 x 3 determinant, the cofactors of
// inv() and norm() are evaluated in double from the float entries.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbslam_gpu.h"

namespace orbgpu {

// C = alpha * A (3 x 3) * B (3 x 3)
__host__ __device__ inline void mm3(const float* A, const float* B, float* C, double alpha = 1.0) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double acc =
                ((double)A[r * 3] * B[c] + (double)A[r * 3 + 1] * B[3 + c]) + (double)A[r * 3 + 2] * B[6 + c];
            C[r * 3 + c] = (float)(acc * alpha);
        }
}

// y = alpha * A (3 x 3) * x
__host__ __device__ inline void mv3(const float* A, const float* x, float* y, double alpha = 1.0) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double acc = ((double)A[r * 3] * x[0] + (double)A[r * 3 + 1] * x[1]) + (double)A[r * 3 + 2] * x[2];
        y[r] = (float)(acc * alpha);
    }
}

__host__ __device__ inline void tr3(const float* A, float* At) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) At[r * 3 + c] = A[c * 3 + r];
}

__host__ __device__ inline double det3(const float* m) {
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7],
                 m22 = m[8];
    return (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20);
}

// cv::Mat::inv() of a 3 x 3 (DECOMP_LU closed form); det == 0 gives the zero matrix
__host__ __device__ inline void inv3(const float* S, float* D) {
    double d = det3(S);
    if (d == 0) {
        for (int i = 0; i < 9; i++) D[i] = 0.0f;
        return;
    }
    d = 1.0 / d;
    const double s00 = S[0], s01 = S[1], s02 = S[2], s10 = S[3], s11 = S[4], s12 = S[5], s20 = S[6], s21 = S[7],
                 s22 = S[8];
    D[0] = (float)((s11 * s22 - s12 * s21) * d);
    D[1] = (float)((s02 * s21 - s01 * s22) * d);
    D[2] = (float)((s01 * s12 - s02 * s11) * d);
    D[3] = (float)((s12 * s20 - s10 * s22) * d);
    D[4] = (float)((s00 * s22 - s02 * s20) * d);
    D[5] = (float)((s02 * s10 - s00 * s12) * d);
    D[6] = (float)((s10 * s21 - s11 * s20) * d);
    D[7] = (float)((s01 * s20 - s00 * s21) * d);
    D[8] = (float)((s00 * s11 - s01 * s10) * d);
}

// ---- one Initialize call on the device ------------------------------------------------------
struct InitParams {
    orb_rng rng;   // the caller's stream before the call
    float K[9], T1[9], T2inv[9], T2t[9];
    float sigma;
    int iterations, N, n1;
};

struct InitMotion {
    float R[9], t[3], P2[12], O2[3];
};

struct InitState {   // between the kernels
    int n_hyp, use_H, Nin, pad;
    InitMotion mo[8];
    int nGood[8];
    float parallax[8];
};

struct InitOut {   // head of the result block
    float SH, SF;
    int use_H, best_it_H, best_it_F;
    float H21[9], F21[9];
    int n_hyp, nGood[8];
    float parallax[8];
    int chosen, ok;
    float R21[9], t21[3];
};

struct InitDev {
    const InitParams* par;
    const float4* px;     // N: (u1, v1, u2, v2) in pixels
    const float4* pn;     // N: the same, normalised
    const int* first;     // N: index of the match's key in frame 1
    float* scores;        // 2 * iterations: [2 it + model], model 0 = H, 1 = F
    float* mats;          // 2 * iterations x 18: H21 | H12, or F21 | 0
    InitState* st;
    uint32_t* keys;       // 8 x N: order-preserving keys of the accepted cosines
    float* P3D;           // 8 x n1 x 3
    uint8_t* good;        // 8 x n1
    InitOut* out;
    float* vP3D;          // n1 x 3
    uint8_t* tri;         // n1
    uint8_t* maskH;       // N
    uint8_t* maskF;       // N
};

// the four launches of one call on stream s; ev: 5 events recorded around them, or nullptr
int initializer_launch(const InitDev& D, int iterations, hipStream_t s, hipEvent_t* ev);

}  // namespace orbgpu
