// svd4.hpp -- the 4 x 4 float SVD of a linear triangulation (LocalMapping::CreateNewMapPoints,
// Initializer::Triangulate), one thread per system.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace orbgpu {

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4 x 4 CV_32F A, reduced to what
// CreateNewMapPoints reads: vt.row(3).  OpenCV 3.2 JacobiSVDImpl_<float> on At = A^T (m >= n:
// the source is transposed, vt is the rotation accumulator): float storage; W, the dot products
// and the rotation scalars in double; sqrt(p^2 + beta^2) for hypot as in epnp.hpp; eps =
// 2 * FLT_EPSILON; 30 sweeps at most; rotated elements rounded to float.  The final pass that
// re-normalises the rows of At for singular values <= FLT_MIN touches u only and is dropped.
// Every index is static: At, Vt and W stay in registers.
__device__ __forceinline__ void svd4_vt3(float (&At)[4][4], float (&x)[4]) {
    const double eps = (double)(FLT_EPSILON * 2);
    double W[4];
    float Vt[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd += (double)At[i][k] * At[i][k];
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < 4; k++) Vt[i][k] = k == i ? 1.0f : 0.0f;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; k++) p += (double)At[i][k] * At[j][k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = (float)(c * At[i][k] + s * At[j][k]);
                    const float t1 = (float)(-s * At[i][k] + c * At[j][k]);
                    At[i][k] = t0;
                    At[j][k] = t1;
                    a += (double)t0 * t0;
                    b += (double)t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = (float)(c * Vt[i][k] + s * Vt[j][k]);
                    const float t1 = (float)(-s * Vt[i][k] + c * Vt[j][k]);
                    Vt[i][k] = t0;
                    Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd += (double)At[i][k] * At[i][k];
        W[i] = sqrt(sd);
    }
    // descending selection sort (strict '<': the earliest of equal values stays), rows swapped
    // through selects over the static candidates
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (wj < W[k]) {
                j = k;
                wj = W[k];
            }
#pragma unroll
        for (int r = i + 1; r < 4; r++) {
            const bool sw = j == r;
            const double tw = W[i];
            W[i] = sw ? W[r] : W[i];
            W[r] = sw ? tw : W[r];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float t = Vt[i][k];
                Vt[i][k] = sw ? Vt[r][k] : Vt[i][k];
                Vt[r][k] = sw ? t : Vt[r][k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] = Vt[3][k];
}

}  // namespace orbgpu
