// sim3_math.hpp -- g2o::Sim3 arithmetic (sim3.h) as explicit IEEE operation sequences, shared by
// OptimizeSim3 (sim3opt.hip) and OptimizeEssentialGraph (essgraph.hip): exp, product, inverse
// (bit-identical to oracle/ba.c ora_sim3_*), and log / map for the pose graph.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_math.hpp"
#include "detmath.hpp"

namespace orbgpu {

struct Sim3d {   // g2o::Sim3: q = (x, y, z, w) like Eigen coeffs(), t, s
    double q[4];
    double t[3];
    double s;
};

// g2o::Sim3(const Vector7d& update)  sim3.h:64-146
__device__ __forceinline__ void sim3_exp(const double* upd, Sim3d& o) {
    const double w0 = upd[0], w1 = upd[1], w2 = upd[2];
    const double sigma = upd[6];
    const double theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double Om2[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            Om2[i * 3 + j] = (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
    const double s = detmath::exp_d(sigma);
    const double eps = 0.00001;
    double A, B, C, ra = 1.0, rb = 1.0;
    const bool small = theta < eps;
    if (!small) {
        double sn, cs;
        detmath::sincos_d(theta, &sn, &cs);
        ra = sn / theta;
        rb = (1 - cs) / (theta * theta);
        if (fabs(sigma) < eps) {
            C = 1;
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        } else {
            C = (s - 1) / sigma;
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    } else if (fabs(sigma) < eps) {
        C = 1;
        A = 1. / 2.;
        B = 1. / 6.;
    } else {
        C = (s - 1) / sigma;
        const double sigma2 = sigma * sigma;
        A = ((sigma - 1) * s + 1) / sigma2;
        B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4) == 0 ? 1.0 : 0.0;
        R[i] = small ? (I + Om[i]) + Om2[i] : (I + ra * Om[i]) + rb * Om2[i];
    }
    quat_from_R(R, o.q);
    double W[9];
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = (A * Om[i] + B * Om2[i]) + C * ((i % 4) == 0 ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = (W[i * 3] * upd[3] + W[i * 3 + 1] * upd[4]) + W[i * 3 + 2] * upd[5];
    o.s = s;
}

// operator*  sim3.h:264-270
__device__ __forceinline__ void sim3_mul(const Sim3d& a, const Sim3d& b, Sim3d& o) {
    Sim3d r;
    r.q[3] = ((a.q[3] * b.q[3] - a.q[0] * b.q[0]) - a.q[1] * b.q[1]) - a.q[2] * b.q[2];
    r.q[0] = ((a.q[3] * b.q[0] + a.q[0] * b.q[3]) + a.q[1] * b.q[2]) - a.q[2] * b.q[1];
    r.q[1] = ((a.q[3] * b.q[1] + a.q[1] * b.q[3]) + a.q[2] * b.q[0]) - a.q[0] * b.q[2];
    r.q[2] = ((a.q[3] * b.q[2] + a.q[2] * b.q[3]) + a.q[0] * b.q[1]) - a.q[1] * b.q[0];
    double rt[3];
    quat_rotate(a.q, b.t, rt);
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    o = r;
}

// inverse  sim3.h:235-238
__device__ __forceinline__ void sim3_inverse(const Sim3d& T, Sim3d& o) {
    Sim3d r;
    r.q[0] = -T.q[0];
    r.q[1] = -T.q[1];
    r.q[2] = -T.q[2];
    r.q[3] = T.q[3];
    const double ms = -1. / T.s;
    const double v[3] = {ms * T.t[0], ms * T.t[1], ms * T.t[2]};
    quat_rotate(r.q, v, r.t);
    r.s = 1. / T.s;
    o = r;
}

// Sim3::log  sim3.h:148-226: (omega, upsilon, sigma), the inverse of sim3_exp with the same
// A, B, C (g2o's B of the theta ~ 0, sigma != 0 branch as it stands); upsilon = W^-1 t by
// cofactors (W = A Omega + B Omega^2 + C I is C I plus a small or skew part: well conditioned)
__device__ __forceinline__ void sim3_log(const Sim3d& T, double* res) {
    const double s = T.s;
    const double sigma = detmath::log_d(s);
    double R[9];
    quat_to_R(T.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR
    const double eps = 0.00001;
    const bool nearI = d > 1 - eps;
    double A, B, C, k = 0.5;
    if (fabs(sigma) < eps) {
        C = 1;
        if (nearI) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(fmax(d, -1.0));
            const double theta2 = theta * theta;
            k = theta / (2 * sqrt(1 - d * d));
            double sn, cs;
            detmath::sincos_d(theta, &sn, &cs);
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (nearI) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(fmax(d, -1.0));
            k = theta / (2 * sqrt(1 - d * d));
            const double theta2 = theta * theta;
            double sn, cs;
            detmath::sincos_d(theta, &sn, &cs);
            const double a = s * sn, b = s * cs;
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double w0 = k * dR[0], w1 = k * dR[1], w2 = k * dR[2];
    const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double W[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double o2 = (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
            W[i * 3 + j] = (A * Om[i * 3 + j] + B * o2) + (i == j ? C : 0.0);
        }
    // rows of adj(W)^T: c0 = W1 x W2, c1 = W2 x W0, c2 = W0 x W1 (W_i the rows); x_j = (t . column j cofactors) / det
    double c0[3], c1[3], c2[3];
    cross3(W + 3, W + 6, c0);
    cross3(W + 6, W, c1);
    cross3(W, W + 3, c2);
    const double det = (W[0] * c0[0] + W[1] * c0[1]) + W[2] * c0[2];
    res[0] = w0;
    res[1] = w1;
    res[2] = w2;
#pragma unroll
    for (int j = 0; j < 3; j++) res[3 + j] = ((c0[j] * T.t[0] + c1[j] * T.t[1]) + c2[j] * T.t[2]) / det;
    res[6] = sigma;
}

// Sim3::map  sim3.h:228-231: s (r * xyz) + t
__device__ __forceinline__ void sim3_map(const Sim3d& T, const double* X, double* out) {
    double r[3];
    quat_rotate(T.q, X, r);
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = T.s * r[i] + T.t[i];
}

}  // namespace orbgpu
