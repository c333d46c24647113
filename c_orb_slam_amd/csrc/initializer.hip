// initializer.hip -- gfx950 kernels of ORB_SLAM2::Initializer::Initialize (src/Initializer.cc):
//   k_init_hypotheses  FindHomography / FindFundamental: one workgroup (one wave) per (model,
//                      iteration) draws its 8-point set, solves the 16 x 9 or 8 x 9 system with
//                      OpenCV's float Jacobi SVD and scores every match.
//   k_init_select      the winning iteration of each model, RH, the winners' inlier masks and the
//                      motion hypotheses (DecomposeE x 4 or the eight Faugeras solutions).
//   k_init_check_rt    CheckRT, one workgroup per motion hypothesis, a thread per match.
//   k_init_finish      ReconstructF's / ReconstructH's acceptance rules and the outputs.
// Float expressions follow the reference's operation order (-ffp-contract=off, correctly rounded
// f32 div/sqrt); the small matrices follow OpenCV (initializer.hpp).  Every sum whose order the
// reference fixes is evaluated in that order: the scores by a sequential float sum over the terms
// in match order, the SVD's dot products over k ascending.  Counts are integers and the parallax
// is a rank selection, so neither depends on the launch geometry.
#include <cfloat>

#include "detmath.hpp"
#include "initializer.hpp"
#include "orb_common.hpp"
#include "ransac_dev.hpp"
#include "svd4.hpp"

namespace orbgpu {

namespace {

constexpr int kSA = 16;   // row stride of At in LDS
constexpr int kSV = 9;    // row stride of Vt in LDS

// cv::RNG(0x12345678).next(): multiply-with-carry
__device__ __forceinline__ unsigned cvrng_next(unsigned long long& state) {
    state = (unsigned long long)(unsigned)state * 4164903690ull + (unsigned)(state >> 32);
    return (unsigned)state;
}

// OpenCV 3.2 JacobiSVDImpl_<float> (oracle/linalg.c jacobi_svd with float storage) run by one
// wave on LDS: At holds n1 rows of length m (rows n.. zero), the first n are orthogonalised in
// cyclic order; Vt (n x n, may be null) accumulates the rotations; W (n doubles) receives the
// singular values, descending.  Lane k owns column k of At and of Vt and rotates it; every lane
// evaluates the double dot products itself from broadcast LDS reads over k ascending, so no
// reduction is involved and the order is OpenCV's.  W, the dot products and the rotation
// scalars are double, eps = 2 * FLT_EPSILON, hypot = sqrt(p^2 + beta^2), rotated and scaled
// entries are rounded to float.  normalise: the final pass over the first n1 rows (division by
// the singular value; a row with W <= FLT_MIN is rebuilt from cv::RNG(0x12345678) and two
// Gram-Schmidt passes) -- only the callers that read those rows ask for it.
// Every lane of the 64-thread workgroup calls it; data is final after it returns.
__device__ void jacobi_wave(float* At, float* Vt, double* W, int m, int n, int n1, bool normalise) {
    const int k = threadIdx.x;
    const double eps = (double)(FLT_EPSILON * 2);
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int q = 0; q < m; q++) sd += (double)At[i * kSA + q] * At[i * kSA + q];
        if (k == 0) W[i] = sd;
    }
    if (Vt)
        for (int e = k; e < n * n; e += 64) Vt[(e / n) * kSV + e % n] = e / n == e % n ? 1.0f : 0.0f;
    __syncthreads();
    const int max_iter = m > 30 ? m : 30;
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                const float* Ai = At + i * kSA;
                const float* Aj = At + j * kSA;
                double a = W[i], p = 0, b = W[j];
                for (int q = 0; q < m; q++) p += (double)Ai[q] * Aj[q];
                if (fabs(p) <= eps * sqrt(a * b)) continue;   // the same in every lane
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
                float t0 = 0, t1 = 0, v0 = 0, v1 = 0;
                if (k < m) {
                    const float ai = Ai[k], aj = Aj[k];
                    t0 = (float)(c * ai + s * aj);
                    t1 = (float)(-s * ai + c * aj);
                }
                if (Vt && k < n) {
                    const float vi = Vt[i * kSV + k], vj = Vt[j * kSV + k];
                    v0 = (float)(c * vi + s * vj);
                    v1 = (float)(-s * vi + c * vj);
                }
                __syncthreads();   // every lane has read rows i and j
                if (k < m) {
                    At[i * kSA + k] = t0;
                    At[j * kSA + k] = t1;
                }
                if (Vt && k < n) {
                    Vt[i * kSV + k] = v0;
                    Vt[j * kSV + k] = v1;
                }
                __syncthreads();
                a = b = 0;
                for (int q = 0; q < m; q++) {
                    const float x0 = Ai[q], x1 = Aj[q];
                    a += (double)x0 * x0;
                    b += (double)x1 * x1;
                }
                if (k == 0) {
                    W[i] = a;
                    W[j] = b;
                }
                __syncthreads();
                changed = true;
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int q = 0; q < m; q++) sd += (double)At[i * kSA + q] * At[i * kSA + q];
        __syncthreads();
        if (k == 0) W[i] = sqrt(sd);
    }
    __syncthreads();
    // descending selection sort (strict '<': the earliest of equal values stays)
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int q = i + 1; q < n; q++)
            if (W[j] < W[q]) j = q;
        __syncthreads();
        if (i != j) {
            if (k == 0) {
                const double tw = W[i];
                W[i] = W[j];
                W[j] = tw;
            }
            if (k < m) {
                const float x = At[i * kSA + k];
                At[i * kSA + k] = At[j * kSA + k];
                At[j * kSA + k] = x;
            }
            if (Vt && k < n) {
                const float x = Vt[i * kSV + k];
                Vt[i * kSV + k] = Vt[j * kSV + k];
                Vt[j * kSV + k] = x;
            }
        }
        __syncthreads();
    }
    if (!normalise) return;
    const double minval = (double)FLT_MIN;
    unsigned long long rng = 0x12345678ull;
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? W[i] : 0;
        float* Ai = At + i * kSA;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            // the m pattern words in k order; every lane runs the generator, lane k keeps word k
            const float val0 = (float)(1. / m);
            float mine = 0;
            for (int q = 0; q < m; q++) {
                const float val = (cvrng_next(rng) & 256) != 0 ? val0 : -val0;
                if (q == k) mine = val;
            }
            __syncthreads();
            if (k < m) Ai[k] = mine;
            __syncthreads();
            for (int pass = 0; pass < 2; pass++)
                for (int j = 0; j < i; j++) {
                    const float* Aj = At + j * kSA;
                    sd = 0;
                    for (int q = 0; q < m; q++) sd += (double)Ai[q] * Aj[q];
                    float t = 0;
                    if (k < m) t = (float)((double)Ai[k] - sd * (double)Aj[k]);
                    __syncthreads();
                    if (k < m) Ai[k] = t;
                    __syncthreads();
                    double asum = 0;
                    for (int q = 0; q < m; q++) asum += fabs((double)Ai[q]);
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    if (k < m) t = (float)((double)t * asum);
                    __syncthreads();
                    if (k < m) Ai[k] = t;
                    __syncthreads();
                }
            sd = 0;
            for (int q = 0; q < m; q++) sd += (double)Ai[q] * Ai[q];
            sd = sqrt(sd);
        }
        const double sc = sd > minval ? 1 / sd : 0.;
        float t = 0;
        if (k < m) t = (float)((double)Ai[k] * sc);
        __syncthreads();
        if (k < m) Ai[k] = t;
        __syncthreads();
    }
}

// the table words [8 it, 8 it + 8) of stream g (ransac_dev.hpp's recurrence; the stream up to
// this workgroup's own words is regenerated, a few dozen 31-word steps).  win: 32 u32 of LDS.
__device__ void rng_words8(const orb_rng& g, int it, uint32_t* out8, uint32_t* win) {
    const int lane = threadIdx.x;
    const int from = 8 * it, D = from + 8;
    if (lane < 31) {
        int s = g.f + lane;
        s = s >= 31 ? s - 31 : s;
        win[lane] = (uint32_t)g.tbl[s];
    }
    __syncthreads();
    for (int base = 0; base < D; base += 31) {
        uint32_t v = 0;
        if (lane < 31) {
            v = win[28 + lane % 3];
            for (int j = lane; j >= 0; j -= 3) v += win[j];
        }
        __syncthreads();
        if (lane < 31) {
            win[lane] = v;
            const int w = base + lane;
            if (w >= from && w < D) out8[w - from] = v;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// CheckHomography's two terms of one match; returns bIn
__device__ __forceinline__ bool chi_homography(const float* H, const float* Hi, float4 p, float invS2, float& t1,
                                               float& t2) {
    const float th = 5.991f;
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(Hi[6] * u2 + Hi[7] * v2 + Hi[8]));
    const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
    const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
    const float chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * invS2;
    if (chi1 > th) {
        bIn = false;
        t1 = 0.0f;
    } else {
        t1 = th - chi1;
    }
    const float w1in2inv = (float)(1.0 / (double)(H[6] * u1 + H[7] * v1 + H[8]));
    const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
    const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
    const float chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * invS2;
    if (chi2 > th) {
        bIn = false;
        t2 = 0.0f;
    } else {
        t2 = th - chi2;
    }
    return bIn;
}

// CheckFundamental's two terms of one match; returns bIn
__device__ __forceinline__ bool chi_fundamental(const float* Fm, float4 p, float invS2, float& t1, float& t2) {
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    bool bIn = true;
    const float a2 = Fm[0] * u1 + Fm[1] * v1 + Fm[2];
    const float b2 = Fm[3] * u1 + Fm[4] * v1 + Fm[5];
    const float c2 = Fm[6] * u1 + Fm[7] * v1 + Fm[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invS2;
    if (chi1 > th) {
        bIn = false;
        t1 = 0.0f;
    } else {
        t1 = thScore - chi1;
    }
    const float a1 = Fm[0] * u2 + Fm[3] * v2 + Fm[6];
    const float b1 = Fm[1] * u2 + Fm[4] * v2 + Fm[7];
    const float c1 = Fm[2] * u2 + Fm[5] * v2 + Fm[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invS2;
    if (chi2 > th) {
        bIn = false;
        t2 = 0.0f;
    } else {
        t2 = thScore - chi2;
    }
    return bIn;
}

// cv::SVD::compute(A, w, u, vt, FULL_UV) of a 3 x 3 on the workgroup's LDS arrays
__device__ void svd3_wave(const float* A, float* At, float* Vt, double* W, float* w, float* u, float* vt) {
    const int k = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 9; e++)
        if (k == e) At[(e % 3) * kSA + e / 3] = A[e];   // At = A^T
    __syncthreads();
    jacobi_wave(At, Vt, W, 3, 3, 3, true);
    for (int r = 0; r < 3; r++) {
        w[r] = (float)W[r];
        for (int c = 0; c < 3; c++) {
            u[r * 3 + c] = At[c * kSA + r];
            vt[r * 3 + c] = Vt[r * kSV + c];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double norm3d(const float* v) {
    return sqrt(((double)v[0] * v[0] + (double)v[1] * v[1]) + (double)v[2] * v[2]);
}

// t / cv::norm(t)
__device__ __forceinline__ void unit3(float* t) {
    const float inv = (float)(1.0 / norm3d(t));
    for (int r = 0; r < 3; r++) t[r] = t[r] * inv;
}

// one motion hypothesis with CheckRT's P2 = K [R | t] and O2 = -R^T t
__device__ void emit_motion(InitMotion* mo, const float* R, const float* t, const float* K) {
    if (threadIdx.x != 0) return;
    float Rt[9];
    for (int i = 0; i < 9; i++) mo->R[i] = R[i];
    for (int i = 0; i < 3; i++) mo->t[i] = t[i];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
            mo->P2[r * 4 + c] = (float)(((double)K[r * 3] * b0 + (double)K[r * 3 + 1] * b1) + (double)K[r * 3 + 2] * b2);
        }
    tr3(R, Rt);
    mv3(Rt, t, mo->O2, -1.0);
}

__device__ __forceinline__ float sqrt_or_nan(float x) { return x >= 0 ? sqrtf(x) : __builtin_nanf(""); }

__device__ __forceinline__ double acos_d(double x) { return detmath::atan2_d(sqrt((1.0 - x) * (1.0 + x)), x); }

}  // namespace

__global__ void __launch_bounds__(64) k_init_hypotheses(InitDev D) {
    __shared__ float At[9 * kSA];
    __shared__ float Vt[9 * kSV];
    __shared__ double W[9];
    __shared__ uint32_t win[32], raw[8];
    __shared__ int sidx[8];
    __shared__ float terms[128];
    const InitParams& P = *D.par;
    const int lane = threadIdx.x, it = blockIdx.x >> 1, model = blockIdx.x & 1;
    const int N = P.N;

    rng_words8(P.rng, it, raw, win);
    if (lane == 0) {
        int s[8];
        draw_set<8>(raw, N, s);
#pragma unroll
        for (int i = 0; i < 8; i++) sidx[i] = s[i];
    }
    for (int e = lane; e < 9 * kSA; e += 64) At[e] = 0.0f;
    __syncthreads();
    if (lane < 8) {
        const float4 q = D.pn[sidx[lane]];
        const float u1 = q.x, v1 = q.y, u2 = q.z, v2 = q.w;
        if (model == 0) {
            // ComputeH21: rows 2k and 2k + 1 of the 16 x 9 A; At = A^T
            const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -(u2 * u1), -(u2 * v1), -u2};
#pragma unroll
            for (int c = 0; c < 9; c++) {
                At[c * kSA + 2 * lane] = r0[c];
                At[c * kSA + 2 * lane + 1] = r1[c];
            }
        } else {
            // ComputeF21: row k of the 8 x 9 A (m < n: OpenCV works on A itself)
            const float r0[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
#pragma unroll
            for (int c = 0; c < 9; c++) At[lane * kSA + c] = r0[c];
        }
    }
    __syncthreads();

    float M[9], M21[9], M12[9], tmp[9];
    if (model == 0) {
        jacobi_wave(At, Vt, W, 16, 9, 9, false);
#pragma unroll
        for (int c = 0; c < 9; c++) M[c] = Vt[8 * kSV + c];
        mm3(P.T2inv, M, tmp);
        mm3(tmp, P.T1, M21);
        inv3(M21, M12);
    } else {
        jacobi_wave(At, nullptr, W, 9, 8, 9, true);
        float Fpre[9], w[3], u[9], vt[9];
#pragma unroll
        for (int c = 0; c < 9; c++) Fpre[c] = At[8 * kSA + c];
        svd3_wave(Fpre, At, Vt, W, w, u, vt);
        const float Dg[9] = {w[0], 0.0f, 0.0f, 0.0f, w[1], 0.0f, 0.0f, 0.0f, 0.0f};
        mm3(u, Dg, tmp);
        mm3(tmp, vt, M);
        mm3(P.T2t, M, tmp);
        mm3(tmp, P.T1, M21);
#pragma unroll
        for (int c = 0; c < 9; c++) M12[c] = 0.0f;
    }

    // the score: terms in parallel, then the reference's sequential float sum in match order
    // (image-1 term before image-2 term), evaluated by every lane from LDS
    const float invS2 = inv_sigma_square(P.sigma);
    float score = 0.0f;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        float t1 = 0.0f, t2 = 0.0f;
        if (i < N) {
            const float4 p = D.px[i];
            if (model == 0) chi_homography(M21, M12, p, invS2, t1, t2);
            else chi_fundamental(M21, p, invS2, t1, t2);
        }
        terms[2 * lane] = t1;
        terms[2 * lane + 1] = t2;
        __syncthreads();
        const int cnt = 2 * (N - base < 64 ? N - base : 64);
        for (int q = 0; q < cnt; q++) score += terms[q];
        __syncthreads();
    }
    if (lane == 0) D.scores[blockIdx.x] = score;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 9; c++) {
            D.mats[(size_t)blockIdx.x * 18 + c] = M21[c];
            D.mats[(size_t)blockIdx.x * 18 + 9 + c] = M12[c];
        }
    }
}

__global__ void __launch_bounds__(64) k_init_select(InitDev D) {
    __shared__ float At[9 * kSA];
    __shared__ float Vt[9 * kSV];
    __shared__ double W[9];
    __shared__ int sNin;
    const InitParams& P = *D.par;
    const int lane = threadIdx.x, N = P.N;
    if (lane == 0) sNin = 0;

    // strict '>' from 0: the earliest iteration with the greatest score; a NaN never wins
    float SH = 0.0f, SF = 0.0f;
    int bH = -1, bF = -1;
    for (int it = 0; it < P.iterations; it++) {
        const float sh = D.scores[2 * it], sf = D.scores[2 * it + 1];
        if (sh > SH) {
            SH = sh;
            bH = it;
        }
        if (sf > SF) {
            SF = sf;
            bF = it;
        }
    }
    float H21[9], H12[9], F21[9];
#pragma unroll
    for (int c = 0; c < 9; c++) {
        H21[c] = bH >= 0 ? D.mats[(size_t)(2 * bH) * 18 + c] : 0.0f;
        H12[c] = bH >= 0 ? D.mats[(size_t)(2 * bH) * 18 + 9 + c] : 0.0f;
        F21[c] = bF >= 0 ? D.mats[(size_t)(2 * bF + 1) * 18 + c] : 0.0f;
    }
    const float RH = SH / (SH + SF);
    const bool useH = RH > 0.40f;   // a NaN takes the F branch

    const float invS2 = inv_sigma_square(P.sigma);
    int cnt = 0;
    for (int i = lane; i < N; i += 64) {
        const float4 p = D.px[i];
        float t1, t2;
        const bool inH = bH >= 0 && chi_homography(H21, H12, p, invS2, t1, t2);
        const bool inF = bF >= 0 && chi_fundamental(F21, p, invS2, t1, t2);
        D.maskH[i] = inH;
        D.maskF[i] = inF;
        cnt += useH ? inH : inF;
    }
    __syncthreads();
    atomicAdd(&sNin, cnt);
    __syncthreads();

    InitState* st = D.st;
    InitOut* out = D.out;
    int n_hyp = 0;
    const float* K = P.K;
    float tmp[9], A[9], w[3], U[9], Vt3[9];
    if (useH && bH >= 0) {
        // ReconstructH: the eight solutions of Faugeras' decomposition of A = K^-1 H21 K
        float invK[9];
        inv3(K, invK);
        mm3(invK, H21, tmp);
        mm3(tmp, K, A);
        svd3_wave(A, At, Vt, W, w, U, Vt3);
        const float s = (float)(det3(U) * det3(Vt3));
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        if (!((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001)) {
            const float q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
            const float den = q1 - q3;
            const float aux1 = sqrt_or_nan((q1 - q2) / den);
            const float aux3 = sqrt_or_nan((q2 - q3) / den);
            const float x1[4] = {aux1, aux1, -aux1, -aux1};
            const float x3[4] = {aux3, -aux3, aux3, -aux3};
            const float root = sqrt_or_nan((q1 - q2) * (q2 - q3));
            for (int cs = 0; cs < 2; cs++) {
                const float den2 = cs == 0 ? (d1 + d3) * d2 : (d1 - d3) * d2;
                const float sn = root / den2;
                const float co = cs == 0 ? (q2 + d1 * d3) / den2 : (d1 * d3 - q2) / den2;
                const float scale = cs == 0 ? d1 - d3 : d1 + d3;
                const float sns[4] = {sn, -sn, -sn, sn};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    float Rp[9], tp[3], R[9], t[3];
                    if (cs == 0) {
                        const float r[9] = {co, 0.0f, -sns[i], 0.0f, 1.0f, 0.0f, sns[i], 0.0f, co};
                        for (int c = 0; c < 9; c++) Rp[c] = r[c];
                        tp[2] = -x3[i] * scale;
                    } else {
                        const float r[9] = {co, 0.0f, sns[i], 0.0f, -1.0f, 0.0f, sns[i], 0.0f, -co};
                        for (int c = 0; c < 9; c++) Rp[c] = r[c];
                        tp[2] = x3[i] * scale;
                    }
                    tp[0] = x1[i] * scale;
                    tp[1] = 0.0f;
                    mm3(U, Rp, tmp, (double)s);
                    mm3(tmp, Vt3, R);
                    mv3(U, tp, t);
                    unit3(t);
                    emit_motion(&st->mo[cs * 4 + i], R, t, K);
                }
            }
            n_hyp = 8;
        }
    } else if (!useH && bF >= 0) {
        // ReconstructF: E21 = K^T F21 K, DecomposeE, (R1, t) (R2, t) (R1, -t) (R2, -t)
        float Kt[9], R1[9], R2[9], t[3], tn[3];
        tr3(K, Kt);
        mm3(Kt, F21, tmp);
        mm3(tmp, K, A);
        svd3_wave(A, At, Vt, W, w, U, Vt3);
        t[0] = U[2];
        t[1] = U[5];
        t[2] = U[8];
        unit3(t);
        const float Wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        float Wt[9];
        tr3(Wm, Wt);
        mm3(U, Wm, tmp);
        mm3(tmp, Vt3, R1);
        if (det3(R1) < 0)
            for (int c = 0; c < 9; c++) R1[c] = -R1[c];
        mm3(U, Wt, tmp);
        mm3(tmp, Vt3, R2);
        if (det3(R2) < 0)
            for (int c = 0; c < 9; c++) R2[c] = -R2[c];
        for (int r = 0; r < 3; r++) tn[r] = -t[r];
        emit_motion(&st->mo[0], R1, t, K);
        emit_motion(&st->mo[1], R2, t, K);
        emit_motion(&st->mo[2], R1, tn, K);
        emit_motion(&st->mo[3], R2, tn, K);
        n_hyp = 4;
    }
    if (lane == 0) {
        st->n_hyp = n_hyp;
        st->use_H = useH;
        st->Nin = sNin;
        for (int h = 0; h < 8; h++) {
            st->nGood[h] = 0;
            st->parallax[h] = 0.0f;
        }
        out->SH = SH;
        out->SF = SF;
        out->use_H = useH;
        out->best_it_H = bH;
        out->best_it_F = bF;
        for (int c = 0; c < 9; c++) {
            out->H21[c] = H21[c];
            out->F21[c] = F21[c];
        }
        out->n_hyp = n_hyp;
    }
}

// order-preserving map of a non-NaN float onto uint32 and back
__device__ __forceinline__ uint32_t float_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(256) k_init_check_rt(InitDev D) {
    __shared__ int sGood, sCnt;
    const InitParams& P = *D.par;
    InitState* st = D.st;
    const int h = blockIdx.x, tid = threadIdx.x;
    if (h >= st->n_hyp) return;
    const int N = P.N, n1 = P.n1;
    const InitMotion& mo = st->mo[h];
    float R[9], t[3], P2[12], O2[3];
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = mo.R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        t[c] = mo.t[c];
        O2[c] = mo.O2[c];
    }
#pragma unroll
    for (int c = 0; c < 12; c++) P2[c] = mo.P2[c];
    const float fx = P.K[0], fy = P.K[4], cx = P.K[2], cy = P.K[5];
    float P1[12];   // K [I | 0]
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) P1[r * 4 + c] = P.K[r * 3 + c];
        P1[r * 4 + 3] = 0.0f;
    }
    const float th2 = (float)(4.0 * (double)(P.sigma * P.sigma));
    const uint8_t* mask = st->use_H ? D.maskH : D.maskF;
    float* P3D = D.P3D + (size_t)h * n1 * 3;
    uint8_t* good = D.good + (size_t)h * n1;
    uint32_t* keys = D.keys + (size_t)h * N;

    if (tid == 0) sGood = 0;
    for (int i = tid; i < n1 * 3; i += 256) P3D[i] = 0.0f;
    for (int i = tid; i < n1; i += 256) good[i] = 0;
    __syncthreads();

    int nLocal = 0;
    for (int i = tid; i < N; i += 256) {
        uint32_t key = 0xffffffffu;   // above every cosine's key
        if (mask[i]) {
            const float4 p = D.px[i];
            float At[4][4], v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                At[k][0] = p.x * P1[8 + k] - P1[k];
                At[k][1] = p.y * P1[8 + k] - P1[4 + k];
                At[k][2] = p.z * P2[8 + k] - P2[k];
                At[k][3] = p.w * P2[8 + k] - P2[4 + k];
            }
            svd4_vt3(At, v);
            const float inv = (float)(1.0 / (double)v[3]);
            const float X[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
            bool ok = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
            float cosP = 0.0f;
            if (ok) {
                const float dist1 = (float)norm3d(X);
                const float n2[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};
                const float dist2 = (float)norm3d(n2);
                const double dot = ((double)X[0] * n2[0] + (double)X[1] * n2[1]) + (double)X[2] * n2[2];
                cosP = (float)(dot / (double)(dist1 * dist2));
                // a NaN cosine (a point on a camera centre) would make the reference's sort undefined
                ok = cosP == cosP;
            }
            const bool lowPar = (double)cosP < 0.99998;
            if (ok && X[2] <= 0 && lowPar) ok = false;
            float X2[3];
#pragma unroll
            for (int r = 0; r < 3; r++)
                X2[r] = (float)((((double)R[r * 3] * X[0] + (double)R[r * 3 + 1] * X[1]) + (double)R[r * 3 + 2] * X[2]) +
                                (double)t[r]);
            if (ok && X2[2] <= 0 && lowPar) ok = false;
            if (ok) {
                const float invZ1 = (float)(1.0 / (double)X[2]);
                const float ex = (fx * X[0] * invZ1 + cx) - p.x, ey = (fy * X[1] * invZ1 + cy) - p.y;
                if (ex * ex + ey * ey > th2) ok = false;
            }
            if (ok) {
                const float invZ2 = (float)(1.0 / (double)X2[2]);
                const float ex = (fx * X2[0] * invZ2 + cx) - p.z, ey = (fy * X2[1] * invZ2 + cy) - p.w;
                if (ex * ex + ey * ey > th2) ok = false;
            }
            if (ok) {
                const int f = D.first[i];
                P3D[3 * f] = X[0];
                P3D[3 * f + 1] = X[1];
                P3D[3 * f + 2] = X[2];
                good[f] = lowPar;
                key = float_key(cosP);
                nLocal++;
            }
        }
        keys[i] = key;
    }
    atomicAdd(&sGood, nLocal);
    __syncthreads();
    const int nGood = sGood;
    float parallax = 0.0f;
    if (nGood > 0) {
        // the cosine of rank min(50, nGood - 1) in ascending order: a radix select on the keys,
        // integer counts only
        int idx = nGood - 1 < 50 ? nGood - 1 : 50;
        uint32_t prefix = 0;
        for (int bit = 31; bit >= 0; bit--) {
            if (tid == 0) sCnt = 0;
            __syncthreads();
            int c = 0;
            for (int i = tid; i < N; i += 256) c += ((keys[i] ^ prefix) >> bit) == 0;
            if (c) atomicAdd(&sCnt, c);
            __syncthreads();
            const int zeros = sCnt;
            if (idx >= zeros) {
                idx -= zeros;
                prefix |= 1u << bit;
            }
            __syncthreads();
        }
        parallax = (float)(acos_d((double)key_float(prefix)) * 180 / 3.1415926535897932384626433832795);
    }
    if (tid == 0) {
        st->nGood[h] = nGood;
        st->parallax[h] = parallax;
    }
}

__global__ void __launch_bounds__(256) k_init_finish(InitDev D) {
    const InitParams& P = *D.par;
    const InitState* st = D.st;
    InitOut* out = D.out;
    const int tid = threadIdx.x, n1 = P.n1, n_hyp = st->n_hyp, Nin = st->Nin;
    int chosen = -1;
    if (n_hyp == 8) {
        // ReconstructH (minParallax 1.0, minTriangulated 50)
        int best = 0, second = 0, bi = -1;
        float bpar = -1.0f;
        for (int k = 0; k < 8; k++) {
            const int g = st->nGood[k];
            if (g > best) {
                second = best;
                best = g;
                bi = k;
                bpar = st->parallax[k];
            } else if (g > second) {
                second = g;
            }
        }
        if ((double)second < 0.75 * best && bpar >= 1.0f && best > 50 && (double)best > 0.9 * Nin) chosen = bi;
    } else if (n_hyp == 4) {
        // ReconstructF
        int mx = 0;
        for (int k = 0; k < 4; k++) mx = st->nGood[k] > mx ? st->nGood[k] : mx;
        const int n09 = (int)(0.9 * Nin);
        const int nMinGood = n09 > 50 ? n09 : 50;
        int nsimilar = 0;
        for (int k = 0; k < 4; k++) nsimilar += (double)st->nGood[k] > 0.7 * mx;
        if (!(mx < nMinGood || nsimilar > 1)) {
            int k = 0;
            while (st->nGood[k] != mx) k++;
            if (st->parallax[k] > 1.0f) chosen = k;
        }
    }
    if (tid == 0) {
        for (int k = 0; k < 8; k++) {
            out->nGood[k] = k < n_hyp ? st->nGood[k] : 0;
            out->parallax[k] = k < n_hyp ? st->parallax[k] : 0.0f;
        }
        out->chosen = chosen;
        out->ok = chosen >= 0;
        for (int c = 0; c < 9; c++) out->R21[c] = chosen >= 0 ? st->mo[chosen].R[c] : 0.0f;
        for (int c = 0; c < 3; c++) out->t21[c] = chosen >= 0 ? st->mo[chosen].t[c] : 0.0f;
    }
    if (chosen < 0) return;
    const float* P3D = D.P3D + (size_t)chosen * n1 * 3;
    const uint8_t* good = D.good + (size_t)chosen * n1;
    for (int i = tid; i < n1 * 3; i += 256) D.vP3D[i] = P3D[i];
    for (int i = tid; i < n1; i += 256) D.tri[i] = good[i];
}

int initializer_launch(const InitDev& D, int iterations, hipStream_t s, hipEvent_t* ev) {
    if (ev) ORB_HIP_CHECK(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(k_init_hypotheses, dim3(2 * iterations), dim3(64), 0, s, D);
    ORB_HIP_CHECK(hipGetLastError());
    if (ev) ORB_HIP_CHECK(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(k_init_select, dim3(1), dim3(64), 0, s, D);
    ORB_HIP_CHECK(hipGetLastError());
    if (ev) ORB_HIP_CHECK(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(k_init_check_rt, dim3(8), dim3(256), 0, s, D);
    ORB_HIP_CHECK(hipGetLastError());
    if (ev) ORB_HIP_CHECK(hipEventRecord(ev[3], s));
    hipLaunchKernelGGL(k_init_finish, dim3(1), dim3(256), 0, s, D);
    ORB_HIP_CHECK(hipGetLastError());
    if (ev) ORB_HIP_CHECK(hipEventRecord(ev[4], s));
    return 0;
}

}  // namespace orbgpu
