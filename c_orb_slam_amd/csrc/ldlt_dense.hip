// ldlt_dense.hip -- the dense single-workgroup LDL^T solvers of the reduced pose system (a local
// BA's n = 6 nP < 144 rows): k_ldlt_reg (register panels, n < 128) and k_ldlt (S in LDS or HBM),
// behind one host entry: dense_ldlt_plan picks the kernel, dense_ldlt_launch launches it.  The four
// rejected A/B kernels (k_ldlt_row / col / t / 2d) remain for unit variants 4-7 of
// debug_ldlt only.  All perform the oracle's ora_ldlt_solve operation sequence per element.
#include <algorithm>
#include <vector>

#include "ba.hpp"
#include "ba_math.hpp"
#include "ldlt.hpp"
#include "orb_common.hpp"

namespace orbgpu {

// Dense LDL^T of the upper triangle + solve, one workgroup (256 threads).
// Same per-element operation sequence as oracle ora_ldlt_solve, blocked by 6-column panels:
// wave 0 factorises the panel rows and writes L (lower triangle), then every wave
// applies the panel's rank-1 updates, in k order, to its trailing rows.
__global__ void __launch_bounds__(256) k_ldlt(int n, double* Sg, const double* bs, double* x, double* scal, int in_lds,
                                              const int* run) {
    BA_GATE(run);
    extern __shared__ double lds[];
    double* y = lds;            // n
    double* A = in_lds ? lds + n : Sg;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    __shared__ int ok;
    if (in_lds)
        for (int q = tid; q < n * n; q += blockDim.x) A[q] = Sg[q];
    for (int q = tid; q < n; q += blockDim.x) y[q] = bs[q];
    if (tid == 0) ok = 1;
    __syncthreads();
    for (int p0 = 0; p0 < n; p0 += 6) {
        const int p1 = min(p0 + 6, n);
        if (w == 0) {
            for (int k = p0; k < p1; k++) {
                const double d = A[(size_t)k * n + k];
                if (d == 0.0) {
                    if (lane == 0) ok = 0;
                    break;
                }
                for (int i = k + 1 + lane; i < n; i += 64) A[(size_t)i * n + k] = A[(size_t)k * n + i] / d;
                __builtin_amdgcn_wave_barrier();
                for (int i = k + 1; i < p1; i++) {
                    const double li = A[(size_t)i * n + k];
                    for (int j = i + lane; j < n; j += 64) A[(size_t)i * n + j] -= li * A[(size_t)k * n + j];
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        if (!ok) break;
        for (int i = p1 + w; i < n; i += 4) {
            double L[6];
            for (int k = p0; k < p1; k++) L[k - p0] = A[(size_t)i * n + k];
            for (int j = i + lane; j < n; j += 64) {
                double v = A[(size_t)i * n + j];
                for (int k = p0; k < p1; k++) v -= L[k - p0] * A[(size_t)k * n + j];
                A[(size_t)i * n + j] = v;
            }
        }
        __syncthreads();
    }
    if (!ok) {
        if (tid == 0) scal[3] = 0.0;
        return;
    }
    if (w == 0) {
        // L y = b: per row, subtractions in k order (column-sweep order of the oracle)
        for (int r0 = 0; r0 < n; r0 += 64) {
            const int i = r0 + lane;
            double acc = i < n ? y[i] : 0.0;
            for (int k = 0; k < r0; k++)
                if (i < n) acc -= A[(size_t)i * n + k] * y[k];
            for (int k = r0; k < min(r0 + 64, n); k++) {
                const double yk = __shfl(acc, k - r0, 64);
                if (i > k && i < n) acc -= A[(size_t)i * n + k] * yk;
            }
            if (i < n) y[i] = acc;
            __builtin_amdgcn_wave_barrier();
        }
        for (int k = lane; k < n; k += 64) y[k] = y[k] / A[(size_t)k * n + k];
        __builtin_amdgcn_wave_barrier();
        // L^T x = z: per row, subtractions in descending k order
        for (int r1 = n; r1 > 0; r1 -= 64) {
            const int r0 = max(r1 - 64, 0);
            const int i = r0 + lane;
            double acc = i < r1 ? y[i] : 0.0;
            for (int k = n - 1; k >= r1; k--)
                if (i < r1) acc -= A[(size_t)k * n + i] * y[k];
            for (int k = r1 - 1; k >= r0; k--) {
                const double yk = __shfl(acc, k - r0, 64);
                if (i < k) acc -= A[(size_t)k * n + i] * yk;
            }
            if (i < r1) y[i] = acc;
            __builtin_amdgcn_wave_barrier();
        }
        for (int k = lane; k < n; k += 64) x[k] = y[k];
        if (lane == 0) scal[3] = 1.0;
    }
}

__device__ __forceinline__ double readlane_d(double v, int l) {
    const unsigned long long u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(u & 0xffffffffu), l);
    const int hi = __builtin_amdgcn_readlane((int)(u >> 32), l);
    return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// z = D^-1 y, then L^T x = z (per row, subtractions in descending k order; L[k][i] =
// Lall[i * n + k]) by one wave; y is overwritten.  The oracle's ora_ldlt_solve sequence.
__device__ __forceinline__ void ldlt_backward_wave(int n, const double* Lall, const double* dvec, double* y, double* x,
                                                   double* scal) {
    const int lane = threadIdx.x & 63;
    for (int k = lane; k < n; k += 64) y[k] = y[k] / dvec[k];
    __builtin_amdgcn_wave_barrier();
    for (int r1 = n; r1 > 0; r1 -= 64) {
        const int r0 = max(r1 - 64, 0);
        const int i = r0 + lane;
        const bool on = i < r1;
        const int ic = on ? i : r0;
        double acc = on ? y[i] : 0.0;
        int k = n - 1;
        for (; k - 8 >= r1 - 1; k -= 8) {
            double L8[8], Y8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                L8[u] = Lall[(size_t)ic * n + (k - u)];
                Y8[u] = y[k - u];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) acc -= L8[u] * Y8[u];
        }
        for (; k >= r1; k--) acc -= Lall[(size_t)ic * n + k] * y[k];
        k = r1 - 1;
        for (; k - 8 >= r0 - 1; k -= 8) {
            double L8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) L8[u] = Lall[(size_t)ic * n + (k - u)];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const double yk = readlane_d(acc, k - u - r0);
                if (i < k - u) acc -= L8[u] * yk;
            }
        }
        for (; k >= r0; k--) {
            const double yk = readlane_d(acc, k - r0);
            if (i < k) acc -= Lall[(size_t)ic * n + k] * yk;
        }
        if (on) y[i] = acc;
        __builtin_amdgcn_wave_barrier();
    }
    for (int k = lane; k < n; k += 64) x[k] = y[k];
    if (lane == 0) scal[3] = 1.0;
}

// Row-owner LDL^T + forward substitution for n <= kLdltRowMax (16 free keyframes: a local BA),
// two waves.  Thread i holds row i of [S | b] (its upper part, j >= i) in registers.  At pivot
// k, row k -- final after its k updates -- sits in LDS (published by its owner at the end of
// pivot k - 1, double-buffered); every row i > k forms l_ik = u_ki / d_k and subtracts
// l_ik * u_kj from each of its entries, k ascending per element: the oracle's ora_ldlt_solve
// sequence (the right-hand side, column n, runs the forward substitution y_i -= l_ik y_k).
// Row k + 1 then publishes itself: one barrier per pivot, no panel round trips.
constexpr int kLdltRowMax = 96;
__global__ void __launch_bounds__(128) k_ldlt_row(int n, const double* __restrict__ Sg, const double* bs, double* x,
                                                  double* scal, const int* run) {
    BA_GATE(run);
    __shared__ double Ur[2][kLdltRowMax + 1];   // published row k: entries j < n, b_k at [kLdltRowMax]
    __shared__ double Lall[kLdltRowMax * kLdltRowMax];   // L[i][k] at Lall[k * n + i]
    __shared__ double dvec[kLdltRowMax], y[kLdltRowMax];
    const int i = threadIdx.x;
    const bool mine = i < n;
    double a[kLdltRowMax];
#pragma unroll
    for (int j = 0; j < kLdltRowMax; j++) a[j] = (mine && j < n && j >= i) ? Sg[(size_t)i * n + j] : 0.0;
    double bi = mine ? bs[i] : 0.0;
    if (i == 0) {
#pragma unroll
        for (int j = 0; j < kLdltRowMax; j++)
            if (j < n) Ur[0][j] = a[j];
        Ur[0][kLdltRowMax] = bi;
    }
    __syncthreads();
    bool ok = true;
    for (int k = 0; k < n; k++) {
        const double* U = Ur[k & 1];
        const double d = U[k];
        if (d == 0.0) {   // uniform: every thread reads the same pivot
            ok = false;
            break;
        }
        if (i == 0) {
            dvec[k] = d;
            y[k] = U[kLdltRowMax];   // b_k after its k updates: forward-substituted y_k
        }
        if (i > k && mine) {
            const double l = U[i] / d;
            Lall[(size_t)k * n + i] = l;
#pragma unroll
            for (int c = 0; c < kLdltRowMax / 8; c++) {
                if (8 * c + 7 < i) continue;
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const int j = 8 * c + q;
                    if (j >= i && j < n) a[j] -= l * U[j];
                }
            }
            bi -= l * U[kLdltRowMax];
            if (i == k + 1) {   // row k + 1 is final: publish it for the next pivot
                double* V = Ur[(k + 1) & 1];
#pragma unroll
                for (int j = 0; j < kLdltRowMax; j++)
                    if (j >= i && j < n) V[j] = a[j];
                V[kLdltRowMax] = bi;
            }
        }
        __syncthreads();
    }
    if (!ok) {
        if (i == 0) scal[3] = 0.0;
        return;
    }
    if (i >= 64) return;
    ldlt_backward_wave(n, Lall, dvec, y, x, scal);
}

// Column-owner LDL^T + solve for n <= kLdltColMax (16 free keyframes: a local BA), 4 waves.
// Lane c owns columns c and c + 64 of [S | b] (b in column n); wave w owns rows i = 4 r + w,
// so a thread holds A[i][c] for its wave's rows in registers.  Pivot k: the pivot row (final
// after k updates) sits in LDS, published by its owner at the end of pivot k - 1 (double-
// buffered); every thread forms l_ck = u_kc / d_k for its columns (two lane-parallel quotients,
// one reciprocal), the wave reads back the l of its own rows, and subtracts l_ik u_kj from its
// rows, k ascending per element: the oracle's ora_ldlt_solve sequence (column n runs the
// forward substitution y_i -= l_ik y_k).  The owner of row k + 1 updates that row first and
// publishes it, one barrier per pivot.  The pivot loop is rolled: its body (24 rows x 2
// columns) stays in the instruction cache, unlike a fully unrolled 90-pivot chain.
constexpr int kLdltColMax = 96;
constexpr int kLdltColRows = kLdltColMax / 4;
__global__ void __launch_bounds__(256) k_ldlt_col(int n, const double* __restrict__ Sg, const double* bs, double* x,
                                                  double* scal, const int* run) {
    BA_GATE(run);
    __shared__ double Ur[2][128];                        // published row k: columns 0..n (b at n)
    __shared__ double Lall[kLdltColMax * kLdltColMax];   // L[i][k] at Lall[k * n + i]
    __shared__ __attribute__((aligned(16))) double lw[4][kLdltColRows + 8];   // l_ik of wave w's rows (r = i / 4)
    __shared__ double dvec[kLdltColMax], y[kLdltColMax];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c0 = lane, c1 = lane + 64;
    double A0[kLdltColRows], A1[kLdltColRows];
#pragma unroll
    for (int r = 0; r < kLdltColRows; r++) {
        const int i = 4 * r + w;
        const bool row = i < n;
        A0[r] = (row && c0 < n && c0 >= i) ? Sg[(size_t)i * n + c0] : (row && c0 == n) ? bs[i] : 0.0;
        A1[r] = (row && c1 < n && c1 >= i) ? Sg[(size_t)i * n + c1] : (row && c1 == n) ? bs[i] : 0.0;
    }
    if (w == 0) {
        Ur[0][c0] = A0[0];
        Ur[0][c1] = A1[0];
    }
    __syncthreads();
    bool ok = true;
    for (int k = 0; k < n; k++) {
        const double* U = Ur[k & 1];
        double* V = Ur[(k + 1) & 1];
        const double d = U[k];
        if (d == 0.0) {   // uniform: every thread reads the same pivot
            ok = false;
            break;
        }
        const double u0 = U[c0], u1 = U[c1];
        const int own = (k + 1) & 3;   // the wave of row k + 1
        if (w == own) {
            // row k + 1 first: its l from the broadcast u_{k,k+1} (the same quotient lane k + 1 forms)
            const int r1 = (k + 1) >> 2;
            const double l1 = U[k + 1 < n ? k + 1 : k] / d;
#pragma unroll
            for (int r = 0; r < kLdltColRows; r++)
                if (r == r1 && k + 1 < n) {
                    A0[r] -= l1 * u0;
                    A1[r] -= l1 * u1;
                    V[c0] = A0[r];
                    V[c1] = A1[r];
                }
        }
        // plain divisions: two cost 160 cycles, one reciprocal shared by two 324
        // (tools/micro/ldlt_col.hip)
        const double l0 = u0 / d, l1v = u1 / d;
        if (w == 0) {
            if (c0 > k && c0 < n) Lall[k * n + c0] = l0;
            if (c1 > k && c1 < n) Lall[k * n + c1] = l1v;
            if (lane == 0) {
                dvec[k] = d;
                y[k] = U[n];   // b_k after its k updates: the forward-substituted y_k
            }
        }
        if ((lane & 3) == w) {   // the l of this wave's rows, c = 4 r + w
            lw[w][lane >> 2] = l0;
            lw[w][16 + (lane >> 2)] = l1v;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible
        __builtin_amdgcn_wave_barrier();
        // rows i = 4 r + w > k + 1 (row k + 1 was done above), four at a time: a group with a live
        // row loads its four l together and updates branch-free (a branch per row serialised the
        // LDS latency of every row: 2.1 k cycles per pivot, tools/micro/ldlt_col.hip)
        const int rlive = (k + 5 - w) >> 2;   // first r with 4 r + w >= k + 2
#pragma unroll
        for (int g = 0; g < kLdltColRows / 4; g++) {
            if (4 * g + 3 >= rlive && 16 * g + w < n) {
                const double2 la = *reinterpret_cast<const double2*>(&lw[w][4 * g]);
                const double2 lb = *reinterpret_cast<const double2*>(&lw[w][4 * g + 2]);
                const double lv[4] = {la.x, la.y, lb.x, lb.y};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int r = 4 * g + q, i = 4 * r + w;
                    const bool live = i > k + 1 && i < n;
                    const double v0 = A0[r] - lv[q] * u0, v1 = A1[r] - lv[q] * u1;
                    A0[r] = live ? v0 : A0[r];
                    A1[r] = live ? v1 : A1[r];
                }
            }
        }
        __syncthreads();
    }
    if (!ok) {
        if (tid == 0) scal[3] = 0.0;
        return;
    }
    if (w != 0) return;
    ldlt_backward_wave(n, Lall, dvec, y, x, scal);
}

// Row-lane LDL^T + solve for n <= kLdltColMax, 4 waves: lane i owns rows i and i + 64 of
// [S | b] (b in column n), wave w the columns j = 4 r + w (r <= 24).  Pivot k: the published row
// k (final after k updates) sits in LDS, permuted so a wave's columns are contiguous; every lane
// forms its rows' l_ik = u_ki / d_k itself (no l broadcast), reads u_kj of its wave's live
// columns as broadcasts and subtracts l_ik u_kj, k ascending per element: the oracle's
// ora_ldlt_solve sequence (column n runs the forward substitution).  Then lane k + 1 publishes
// its row; one barrier per pivot.  Rows at or above the pivot and lower-triangle entries carry
// values nobody reads, so the updates need no per-row predicate.
constexpr int kLdltTCols = kLdltColMax / 4 + 1;   // 25 columns per wave: j <= 96 covers b at n <= 96
__global__ void __launch_bounds__(256) k_ldlt_t(int n, const double* __restrict__ Sg, const double* bs, double* x,
                                                double* scal, const int* run) {
    BA_GATE(run);
    __shared__ __attribute__((aligned(16))) double Up[2][4][kLdltTCols + 3];   // row k: Up[.][j & 3][j >> 2]
    __shared__ double Lall[kLdltColMax * kLdltColMax];   // S staging, then L[i][k] at Lall[k * n + i]
    __shared__ double dvec[kLdltColMax], y[kLdltColMax];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i0 = lane, i1 = lane + 64;
    // S through LDS: coalesced global reads, then each lane its rows
    for (int q = tid; q < n * n; q += 256) Lall[q] = Sg[q];
    __syncthreads();
    double A0[kLdltTCols], A1[kLdltTCols];
#pragma unroll
    for (int r = 0; r < kLdltTCols; r++) {
        const int j = 4 * r + w;
        A0[r] = (i0 < n && j < n && j >= i0) ? Lall[i0 * n + j] : (i0 < n && j == n) ? bs[i0] : 0.0;
        A1[r] = (i1 < n && j < n && j >= i1) ? Lall[i1 * n + j] : (i1 < n && j == n) ? bs[i1] : 0.0;
    }
    if (lane == 0) {   // row 0
#pragma unroll
        for (int r = 0; r < kLdltTCols; r++) Up[0][w][r] = A0[r];
    }
    __syncthreads();   // the staging area is free for L from here
    bool ok = true;
    for (int k = 0; k < n; k++) {
        const double(*U)[kLdltTCols + 3] = Up[k & 1];
        const double d = U[k & 3][k >> 2];
        if (d == 0.0) {   // uniform
            ok = false;
            break;
        }
        // this lane's rows: l = u_ki / d_k (rows <= k compute values nobody reads)
        const double l0 = k < 63 ? U[i0 & 3][i0 >> 2] / d : 0.0;
        const double l1 = n > 64 ? U[i1 & 3][i1 >> 2] / d : 0.0;
        if (w == 0) {
            if (i0 > k && i0 < n) Lall[k * n + i0] = l0;
            if (i1 > k && i1 < n) Lall[k * n + i1] = l1;
            if (lane == 0) {
                dvec[k] = d;
                y[k] = U[n & 3][n >> 2];   // b_k after its k updates: the forward-substituted y_k
            }
        }
        // live columns j > k of this wave, four at a time (a uniform skip of dead groups)
        const int rlive = (k + 4 - w) >> 2;   // first r with 4 r + w >= k + 1
#pragma unroll
        for (int g = 0; g < (kLdltTCols + 3) / 4; g++) {
            if (4 * g + 3 >= rlive && 16 * g + w <= n) {
                const double2 ua = *reinterpret_cast<const double2*>(&U[w][4 * g]);
                const double2 ub = *reinterpret_cast<const double2*>(&U[w][4 * g + 2]);
                const double uv[4] = {ua.x, ua.y, ub.x, ub.y};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int r = 4 * g + q;
                    if (r < kLdltTCols) {
                        if (k < 63) A0[r] -= l0 * uv[q];
                        if (n > 64) A1[r] -= l1 * uv[q];
                    }
                }
            }
        }
        // row k + 1 is final: its lane publishes this wave's columns
        const int kp = k + 1;
        if (kp < n && (kp < 64 ? lane == kp : lane == kp - 64)) {
            double* V = Up[kp & 1][w];
            if (kp < 64) {   // two loops: a select of the arrays would move them to scratch
#pragma unroll
                for (int r = 0; r < kLdltTCols; r++) V[r] = A0[r];
            } else {
#pragma unroll
                for (int r = 0; r < kLdltTCols; r++) V[r] = A1[r];
            }
        }
        __syncthreads();
    }
    if (!ok) {
        if (tid == 0) scal[3] = 0.0;
        return;
    }
    if (w != 0) return;
    ldlt_backward_wave(n, Lall, dvec, y, x, scal);
}

// 2-D block-cyclic LDL^T + solve for n <= kLdltColMax, 4 waves: thread (a, b) holds A[i][j] for
// i = 16 r + a, j = 16 c + b of [S | b] (b in column n); a wave holds four row classes, so a
// register row or column past the live part of the matrix is skipped by the whole wave.  Per
// panel of 8 pivots: the owners publish the panel rows, wave 0 factors them right-looking
// (lane = column: l_jk = u_kj / d_k lane-parallel, the later panel rows updated with the l read
// back by readlane), writing the final U rows and the L columns to LDS, then every thread
// applies the panel's pivots, ascending, to its live entries.  Per element the oracle's
// ora_ldlt_solve sequence; two barriers per panel.
constexpr int k2dPW = 8, k2dR = 6, k2dC = 7;   // panel width; rows 16 r + a (r < 6), columns 16 c + b (c < 7)
__global__ void __launch_bounds__(256) k_ldlt_2d(int n, const double* __restrict__ Sg, const double* bs, double* x,
                                                 double* scal, const int* run) {
    BA_GATE(run);
    __shared__ double Lall[kLdltColMax * kLdltColMax];   // S staging, then L[i][k] at Lall[k * n + i]
    __shared__ double UP[k2dPW][128];                    // the panel's final U rows, columns 0..n
    __shared__ double Pn[k2dPW][128];                    // the panel rows as published
    __shared__ double dvec[kLdltColMax], y[kLdltColMax];
    __shared__ int ok;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int a = 4 * w + (lane & 3), b = lane >> 2;
    for (int q = tid; q < n * n; q += 256) Lall[q] = Sg[q];
    if (tid == 0) ok = 1;
    __syncthreads();
    double A[k2dR][k2dC];
#pragma unroll
    for (int r = 0; r < k2dR; r++)
#pragma unroll
        for (int c = 0; c < k2dC; c++) {
            const int i = 16 * r + a, j = 16 * c + b;
            A[r][c] = (i < n && j < n && j >= i) ? Lall[i * n + j] : (i < n && j == n) ? bs[i] : 0.0;
        }
    for (int p0 = 0; p0 < n; p0 += k2dPW) {
        const int p1 = min(p0 + k2dPW, n);
        // the panel rows' current values (final: every earlier panel is applied)
#pragma unroll
        for (int r = 0; r < k2dR; r++) {
            const int i = 16 * r + a;
            if (i >= p0 && i < p1)
#pragma unroll
                for (int c = 0; c < k2dC; c++) Pn[i - p0][16 * c + b] = A[r][c];
        }
        __syncthreads();   // also: every thread is done with the previous panel's UP
        if (w == 0) {
            double u0[k2dPW], u1[k2dPW];
#pragma unroll
            for (int t = 0; t < k2dPW; t++) {
                u0[t] = p0 + t < n ? Pn[t][lane] : 0.0;
                u1[t] = p0 + t < n ? Pn[t][lane + 64] : 0.0;
            }
            bool good = true;
#pragma unroll
            for (int t = 0; t < k2dPW; t++) {
                const int k = p0 + t;
                if (k < n && good) {
                    UP[t][lane] = u0[t];   // row k is final
                    UP[t][lane + 64] = u1[t];
                    const double d = k < 64 ? readlane_d(u0[t], k) : readlane_d(u1[t], k - 64);
                    if (d == 0.0) {   // uniform
                        good = false;
                        if (lane == 0) ok = 0;
                    } else {
                        const double l0 = u0[t] / d, l1 = u1[t] / d;   // l_jk, j = lane / lane + 64
                        if (lane > k && lane < n) Lall[k * n + lane] = l0;
                        if (lane + 64 > k && lane + 64 < n) Lall[k * n + lane + 64] = l1;
                        const double yk = n < 64 ? readlane_d(u0[t], n) : readlane_d(u1[t], n - 64);
                        if (lane == 0) {
                            dvec[k] = d;
                            y[k] = yk;   // b_k after its k updates: the forward-substituted y_k
                        }
#pragma unroll
                        for (int t2 = t + 1; t2 < k2dPW; t2++) {
                            const int i = p0 + t2;
                            if (i < n) {
                                const double li = i < 64 ? readlane_d(l0, i) : readlane_d(l1, i - 64);
                                u0[t2] -= li * u0[t];
                                u1[t2] -= li * u1[t];
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (!ok) break;
        // rows >= p1: the panel's pivots, ascending, on the live register rows / columns
        const int pw = p1 - p0;
#pragma unroll
        for (int r = 0; r < k2dR; r++) {
            if (16 * r + 4 * w + 3 < p1) continue;   // the wave's four rows of register row r are done
            const int i = 16 * r + a;
            double lv[k2dPW];
#pragma unroll
            for (int t = 0; t < k2dPW; t++) lv[t] = t < pw ? Lall[(p0 + t) * n + i] : 0.0;
#pragma unroll
            for (int c = 0; c < k2dC; c++) {
                if (16 * c + 15 < p1) continue;      // every column of register column c is done
                const int j = 16 * c + b;
                double v = A[r][c];
#pragma unroll
                for (int t = 0; t < k2dPW; t++)
                    if (t < pw) v -= lv[t] * UP[t][j];
                A[r][c] = v;
            }
        }
    }
    if (!ok) {
        if (tid == 0) scal[3] = 0.0;
        return;
    }
    __syncthreads();
    if (w != 0) return;
    ldlt_backward_wave(n, Lall, dvec, y, x, scal);
}

// The dense LDL^T of the local BA's reduced system (k_ldlt_reg, below).
#ifdef ORB_LDLT_PROBE
__device__ long long g_ldlt_probe[256];
#define LDLT_PROBE(slot) \
    do {                                                  \
        if (threadIdx.x == 0) g_ldlt_probe[slot] = clock64(); \
    } while (0)
#else
#define LDLT_PROBE(slot) \
    do {                 \
    } while (0)
#endif
constexpr int kLdltMax = 128;
constexpr int kLdltWaves = 8;     // 512 threads: 256 VGPRs per lane, the panel registers stay unspilled
constexpr int kLdltThreads = 64 * kLdltWaves;
// LDS of k_ldlt_reg: Lall (n x n), three 6 x kLdltMax panel row buffers, two kLdltMax x 6 panel L
// buffers, d, y
static inline size_t ldlt_reg_shm(int n) { return sizeof(double) * ((size_t)n * n + 1 + 32 * kLdltMax); }

// SharedDiv::div without its branch: the quotient of an in-range numerator, or a * r for a zero
// one (a / b = a signed zero); any other numerator (or an out-of-range divisor) sets `bad` and the
// caller redoes the work with SharedDiv::div.
__device__ __forceinline__ double div_fast(const SharedDiv& d, double a, bool& bad) {
    const double q = a * d.r;
    const double rem = fma(-d.b, q, a);
    const double res = __builtin_amdgcn_div_fixup(fma(rem, d.r, q), d.b, a);
    const double aa = fabs(a);
    const bool inr = aa > 0x1p-300 && aa < 0x1p300;
    bad = bad || !(inr || aa == 0.0);
    return inr ? res : q;
}

// the panel factorisation of k_ldlt_reg for one column thread j, any panel width pw <= 6, with
// SharedDiv::div (the fallback of ldlt_panel6)
__device__ __forceinline__ void ldlt_panel_generic(int n, int p0, int pw, int j, double* U, double* Lall,
                                                   double* Lpan, double* dvec, double* y, int* ok) {
    double Bk[6][6], Lb[6][6], dd[6];
#pragma unroll
    for (int t = 0; t < 6; t++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            Bk[t][c] = (t < pw && c < pw && c >= t) ? U[t * kLdltMax + p0 + c] : 0.0;
            Lb[t][c] = 0.0;
        }
    bool bad = false;
    SharedDiv sd[6] = {SharedDiv(1.0), SharedDiv(1.0), SharedDiv(1.0), SharedDiv(1.0), SharedDiv(1.0),
                       SharedDiv(1.0)};
#pragma unroll
    for (int t = 0; t < 6; t++) {
        dd[t] = Bk[t][t];
        if (t < pw) {
            bad |= dd[t] == 0.0;
            sd[t] = SharedDiv(dd[t]);
#pragma unroll
            for (int t2 = t + 1; t2 < 6; t2++)
                if (t2 < pw) Lb[t2][t] = sd[t].div(Bk[t][t2]);
#pragma unroll
            for (int t2 = t + 1; t2 < 6; t2++)
#pragma unroll
                for (int c = t2; c < 6; c++)
                    if (c < pw) Bk[t2][c] -= Lb[t2][t] * Bk[t][c];
        }
    }
    double u[6];
#pragma unroll
    for (int t = 0; t < 6; t++) u[t] = t < pw ? U[t * kLdltMax + j] : 0.0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        if (t < pw) {
            const int k = p0 + t;
            const bool act = j > k && j < n;
            const double l = act ? sd[t].div(u[t]) : 0.0;
#pragma unroll
            for (int t2 = t + 1; t2 < 6; t2++)
                if (t2 < pw && j >= p0 + t2) u[t2] -= Lb[t2][t] * u[t];
            if (act) {
                Lall[(size_t)k * n + j] = l;
                Lpan[j * 6 + t] = l;
            }
            if (j == n) y[k] = u[t];   // row k's right-hand side is final: forward-substituted y_k
        }
    }
#pragma unroll
    for (int t = 0; t < 6; t++)
        if (t < pw) U[t * kLdltMax + j] = u[t];
    if (j == 0) {
#pragma unroll
        for (int t = 0; t < 6; t++)
            if (t < pw) dvec[p0 + t] = dd[t];
        if (bad) *ok = 0;
    }
}

// A full panel (pw = 6) in one basic block: every thread first factorises the 6x6 diagonal block
// from LDS itself (the same operations as the block's own columns perform, so d and the block's L
// agree bit for bit), then its own column: l_jk = u_kj / d_k and u_tj -= L[t][k] u_kj, k
// ascending.  Results stay in registers until the wave knows that every division was a fast one;
// a wave with a zero pivot or an out-of-range operand redoes the panel with ldlt_panel_generic.
__device__ __forceinline__ void ldlt_panel6(int n, int p0, int j, double* U, double* Lall, double* Lpan,
                                            double* dvec, double* y, int* ok) {
    double B[6][6], Lb[6][6], dd[6];
#pragma unroll
    for (int t = 0; t < 6; t++)
#pragma unroll
        for (int c = t; c < 6; c++) B[t][c] = U[t * kLdltMax + p0 + c];
    double u[6];
#pragma unroll
    for (int t = 0; t < 6; t++) u[t] = U[t * kLdltMax + j];
    bool bad = false;
    SharedDiv sd[6] = {SharedDiv(1.0), SharedDiv(1.0), SharedDiv(1.0), SharedDiv(1.0), SharedDiv(1.0),
                       SharedDiv(1.0)};
#pragma unroll
    for (int t = 0; t < 6; t++) {
        dd[t] = B[t][t];
        sd[t] = SharedDiv(dd[t]);
        bad = bad || !sd[t].ok;
#pragma unroll
        for (int t2 = t + 1; t2 < 6; t2++) Lb[t2][t] = div_fast(sd[t], B[t][t2], bad);
#pragma unroll
        for (int t2 = t + 1; t2 < 6; t2++)
#pragma unroll
            for (int c = t2; c < 6; c++) B[t2][c] -= Lb[t2][t] * B[t][c];
    }
    double l[6];
    bool badc = false;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const bool act = j > p0 + t && j < n;
        bool bt = false;
        const double q = div_fast(sd[t], u[t], bt);
        badc = badc || (act && bt);
        l[t] = act ? q : 0.0;
#pragma unroll
        for (int t2 = t + 1; t2 < 6; t2++) {
            const double v = u[t2] - Lb[t2][t] * u[t];
            u[t2] = j >= p0 + t2 ? v : u[t2];
        }
    }
    if (__ballot(bad || badc)) {
        ldlt_panel_generic(n, p0, 6, j, U, Lall, Lpan, dvec, y, ok);
        return;
    }
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const int k = p0 + t;
        if (j > k && j < n) {
            Lall[(size_t)k * n + j] = l[t];
            Lpan[j * 6 + t] = l[t];
        }
        U[t * kLdltMax + j] = u[t];
    }
    if (j == n)
#pragma unroll
        for (int t = 0; t < 6; t++) y[p0 + t] = u[t];   // forward-substituted y_k
    if (j == 0)
#pragma unroll
        for (int t = 0; t < 6; t++) dvec[p0 + t] = dd[t];
}

// Row waves of k_ldlt_reg (waves 2..7, kRowWaves of them): wave 2 + t owns rows i = 6 r + t
// (slot r < kRowSlots) of columns j = lane, lane + 64, so a 6-row panel p is slot p of every row
// wave.  In phase p a row wave applies panel p - 1's six rank-one updates (its L from Lp, its
// rows u from Up) in k order to its rows i >= 6 (p + 1) -- panel p's own rows were handed to the
// factor waves one phase earlier -- and publishes slot p + 1 (panel p + 1's row, now updated by
// every panel up to p - 1) to Un.  Rows i >= 64 own no column below 64 on or right of the
// diagonal; column registers 64.. matter only for n >= 64 (the right-hand side sits at column n).
constexpr int kRowWaves = 6;
constexpr int kRowSlots = (kLdltMax + kRowWaves - 1) / kRowWaves;
__device__ __forceinline__ void ldlt_rows(double (&R)[2][kRowSlots], const double* Up, const double* Lp, double* Un,
                                          int n, int p1, int t6, int lane) {
    double u0[6], u1[6];
#pragma unroll
    for (int t = 0; t < 6; t++) {
        u0[t] = Up[t * kLdltMax + lane];
        u1[t] = Up[t * kLdltMax + lane + 64];
    }
#pragma unroll
    for (int r = 0; r < kRowSlots; r++) {
        const int i = kRowWaves * r + t6;
        if (i >= p1 && i < n) {
            double L[6];
#pragma unroll
            for (int t = 0; t < 6; t++) L[t] = Lp[i * 6 + t];
            if (i < 64) {
                double v0 = R[0][r];
#pragma unroll
                for (int t = 0; t < 6; t++) v0 -= L[t] * u0[t];
                R[0][r] = lane >= i ? v0 : R[0][r];
            }
            if (n >= 64) {
                double v1 = R[1][r];
#pragma unroll
                for (int t = 0; t < 6; t++) v1 -= L[t] * u1[t];
                R[1][r] = lane + 64 >= i ? v1 : R[1][r];
            }
            if (i < p1 + 6) {   // panel p + 1's row
                Un[(i - p1) * kLdltMax + lane] = R[0][r];
                Un[(i - p1) * kLdltMax + lane + 64] = R[1][r];
            }
        }
    }
}

// Register-resident LDL^T + solve for n < 128 (<= 21 free keyframes), 512 threads, with a
// one-panel lookahead: waves 0-1 factorise 6-column panels (one thread per column j), waves 2-7
// hold the rows.  Phase p: the factor waves factorise panel p from its rows in LDS (every earlier
// panel's updates applied) and signal; the row waves apply panel p - 1 to their rows below panel
// p (the trailing update runs under the factorisation), publish panel p + 1's rows to LDS and,
// once panel p is factored, apply panel p to those rows there (one row per wave, no register
// indexing).  One barrier per phase; panel rows rotate through three buffers, panel L through
// two.  Per-element operation sequence identical to oracle ora_ldlt_solve (every element receives
// the pivots' updates in ascending k).
__global__ void __launch_bounds__(kLdltThreads) k_ldlt_reg(int n, const double* __restrict__ Sg, const double* bs,
                                                           double* x, double* scal, const int* run) {
    BA_GATE(run);
    extern __shared__ double lds[];
    double* Lall = lds;                               // n x n, Lall[k * n + i] = L[i][k]
    double* Ub = Lall + (((size_t)n * n + 1) & ~(size_t)1);   // 3 x (6 x kLdltMax) panel rows (16-B aligned)
    double* Lb = Ub + 18 * kLdltMax;                  // 2 x (kLdltMax x 6) panel L
    double* dvec = Lb + 12 * kLdltMax;                // n
    double* y = dvec + kLdltMax;                      // n
    __shared__ int ok, done;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: row branches stay scalar
    const bool factor = w < kLdltMax / 64;
    const int t6 = w - kLdltMax / 64;
    // [S | b] (n <= 126 < kLdltMax): column n carries the right-hand side, so the row updates run
    // the forward substitution L y = b with the oracle's sequence (y_i -= l_ik y_k, k ascending)
    // and y_k is final when row k becomes a pivot row
    double R[2][kRowSlots];
    if (!factor) {
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int r = 0; r < kRowSlots; r++) {
                const int i = kRowWaves * r + t6, j = lane + 64 * c;
                R[c][r] = (i < n && j < n && i <= j) ? Sg[(size_t)i * n + j] : (i < n && j == n) ? bs[i] : 0.0;
            }
        if (t6 < n) {   // panel 0's rows (slot 0)
            Ub[t6 * kLdltMax + lane] = R[0][0];
            Ub[t6 * kLdltMax + lane + 64] = R[1][0];
        }
    }
    LDLT_PROBE(0);
    if (tid == 0) {
        ok = 1;
        done = 0;
    }
    __syncthreads();
    LDLT_PROBE(1);
    int cur = 0;   // panel p's row buffer: p mod 3
    for (int p0 = 0; p0 < n; p0 += 6) {
        const int p1 = min(p0 + 6, n), pw = p1 - p0, pi = p0 / 6;
        const int prv = cur == 0 ? 2 : cur - 1, nxt = cur == 2 ? 0 : cur + 1;
        double* U = Ub + cur * 6 * kLdltMax;
        double* Un = Ub + nxt * 6 * kLdltMax;
        double* Lpan = Lb + (pi & 1) * 6 * kLdltMax;
        LDLT_PROBE(11 + 4 * (pi < 20 ? pi : 20));
        if (factor) {
            if (pw == 6) ldlt_panel6(n, p0, tid, U, Lall, Lpan, dvec, y, &ok);
            else ldlt_panel_generic(n, p0, pw, tid, U, Lall, Lpan, dvec, y, &ok);
            // (also after a zero pivot: the row waves wait for this count)
            if (lane == 0) __hip_atomic_fetch_add(&done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef ORB_LDLT_PROBE
            if (tid == 0 && pi < 20) g_ldlt_probe[220 + pi] = clock64();   // factor done
#endif
        } else {
            // panel p - 1's updates on the rows below panel p, panel p + 1's rows published.  The
            // slot index is re-made opaque per panel: hoisted out of the panel loop, the rows'
            // offsets and tests spill SGPRs into VGPR lanes (a v_readlane each per row)
            int tv = t6;
            asm volatile("" : "+s"(tv));
            if (p0 > 0) {
                ldlt_rows(R, Ub + prv * 6 * kLdltMax, Lb + ((pi & 1) ^ 1) * 6 * kLdltMax, Un, n, p1, tv, lane);
            } else if (6 + t6 < n) {   // phase 0: panel 1's rows (slot 1) as they are
                Un[t6 * kLdltMax + lane] = R[0][1];
                Un[t6 * kLdltMax + lane + 64] = R[1][1];
            }
#ifdef ORB_LDLT_PROBE
            if (lane == 0 && pi < 16) g_ldlt_probe[124 + 6 * pi + t6] = clock64();   // bulk done
#endif
            const int i = p1 + tv;   // this wave's row of panel p + 1 (panel p is full when it exists)
            if (i < n) {
                while (__hip_atomic_load(&done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < 2 * (pi + 1))
                    __builtin_amdgcn_s_sleep(1);
                double L[6], u0[6], u1[6];
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    L[t] = Lpan[i * 6 + t];
                    u0[t] = U[t * kLdltMax + lane];
                    u1[t] = U[t * kLdltMax + lane + 64];
                }
                double v0 = Un[tv * kLdltMax + lane], v1 = Un[tv * kLdltMax + lane + 64];
                const double o0 = v0, o1 = v1;
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    v0 -= L[t] * u0[t];
                    v1 -= L[t] * u1[t];
                }
                Un[tv * kLdltMax + lane] = lane >= i ? v0 : o0;
                Un[tv * kLdltMax + lane + 64] = lane + 64 >= i ? v1 : o1;
            }
        }
        __syncthreads();
        LDLT_PROBE(12 + 4 * (pi < 20 ? pi : 20));
        if (!ok) break;
        cur = nxt;
    }
    LDLT_PROBE(2);
    if (!ok) {
        if (tid == 0) scal[3] = 0.0;
        return;
    }
    if (w != 0) return;
    LDLT_PROBE(3);
    ldlt_backward_wave(n, Lall, dvec, y, x, scal);
    LDLT_PROBE(4);
}

// ---------------------------------------------------------------- host
// Which kernel solves a system of n rows on a device with ldsMax bytes of LDS per workgroup: the
// register panels below kLdltMax rows (b rides in column n), else the generic kernel with S
// staged in LDS; none when S does not fit (the caller takes the block-sparse solver, ldlt.hip).
DensePlan dense_ldlt_plan(int n, size_t ldsMax) {
    const size_t regShm = ldlt_reg_shm(n);
    if (n < kLdltMax && regShm <= ldsMax) return DensePlan{DenseKernel::Reg, regShm, 0};
    const size_t ldsBytes = sizeof(double) * ((size_t)n + (size_t)n * n);
    if (ldsBytes <= ldsMax) return DensePlan{DenseKernel::Generic, ldsBytes + 16, 1};
    return DensePlan{DenseKernel::None, 0, 0};
}

// The one launch site of k_ldlt_reg and k_ldlt.  ctl: the device LM's gate word, or nullptr.
void dense_ldlt_launch(const DensePlan& plan, int n, double* S, const double* b, double* x, double* scal,
                       const int* ctl, hipStream_t s) {
    if (plan.kernel == DenseKernel::Reg)
        hipLaunchKernelGGL(k_ldlt_reg, dim3(1), dim3(kLdltThreads), plan.shm, s, n, S, b, x, scal, ctl);
    else if (plan.kernel == DenseKernel::Generic)
        hipLaunchKernelGGL(k_ldlt, dim3(1), dim3(256), plan.shm, s, n, S, b, x, scal, plan.in_lds, ctl);
}

// ---------------------------------------------------------------- unit entry points
int debug_ldlt(int n, const double* S, const double* b, double* x, int variant) {
    if (variant == 2 || variant == 3) {   // block-sparse tiled solver (3: nested dissection); upper triangle read
        std::vector<double> U((size_t)n * n, 0.0);
        for (int i = 0; i < n; i++)
            for (int j = i; j < n; j++) U[(size_t)i * n + j] = S[(size_t)i * n + j];
        int ok = 0;
        if (int e = ldlt_sparse_dense(n, U.data(), b, x, &ok, nullptr, variant == 3)) return e < 0 ? e : -1;
        return ok;
    }
    if (variant == 0 && n >= kLdltMax) return -3;   // [S | b] needs a column register for b
    if ((variant == 5 || variant == 6 || variant == 7) && n > kLdltColMax) return -3;
    if (variant == 4 && n > kLdltRowMax) return -3;
    double *dS = nullptr, *dB = nullptr, *dX = nullptr, *dScal = nullptr;
    const size_t nn = (size_t)std::max(n, 1);
    ORB_HIP_CHECK(hipMalloc(&dS, sizeof(double) * nn * nn));
    ORB_HIP_CHECK(hipMalloc(&dB, sizeof(double) * nn));
    ORB_HIP_CHECK(hipMalloc(&dX, sizeof(double) * nn));
    ORB_HIP_CHECK(hipMalloc(&dScal, sizeof(double) * 16));
    ORB_HIP_CHECK(hipMemcpy(dS, S, sizeof(double) * n * n, hipMemcpyHostToDevice));
    ORB_HIP_CHECK(hipMemcpy(dB, b, sizeof(double) * n, hipMemcpyHostToDevice));
    ORB_HIP_CHECK(hipMemset(dX, 0, sizeof(double) * nn));
    // the unit variants name their kernel: 0 the register panels; 4-7 the rejected A/B kernels,
    // which nothing else launches; any other the generic kernel on S in HBM
    if (variant == 4) hipLaunchKernelGGL(k_ldlt_row, dim3(1), dim3(128), 0, 0, n, dS, dB, dX, dScal, nullptr);
    else if (variant == 5) hipLaunchKernelGGL(k_ldlt_col, dim3(1), dim3(256), 0, 0, n, dS, dB, dX, dScal, nullptr);
    else if (variant == 6) hipLaunchKernelGGL(k_ldlt_t, dim3(1), dim3(256), 0, 0, n, dS, dB, dX, dScal, nullptr);
    else if (variant == 7) hipLaunchKernelGGL(k_ldlt_2d, dim3(1), dim3(256), 0, 0, n, dS, dB, dX, dScal, nullptr);
    else if (variant == 0)
        dense_ldlt_launch(DensePlan{DenseKernel::Reg, ldlt_reg_shm(n), 0}, n, dS, dB, dX, dScal, nullptr, nullptr);
    else
        dense_ldlt_launch(DensePlan{DenseKernel::Generic, sizeof(double) * n + 16, 0}, n, dS, dB, dX, dScal, nullptr,
                          nullptr);
    ORB_HIP_CHECK(hipGetLastError());
    double sc[16];
    ORB_HIP_CHECK(hipMemcpy(sc, dScal, sizeof(sc), hipMemcpyDeviceToHost));
    ORB_HIP_CHECK(hipMemcpy(x, dX, sizeof(double) * n, hipMemcpyDeviceToHost));
    (void)hipFree(dS); (void)hipFree(dB); (void)hipFree(dX); (void)hipFree(dScal);
    return sc[3] != 0.0 ? 1 : 0;
}

// tiled factorisation only: A (n x n, upper = S) -> d on the diagonal, L in the strict lower
// triangle, the eliminated rows above
int debug_ldlt_factor(int n, const double* S, double* out) {
    if (n <= 0) return 0;
    std::vector<double> U((size_t)n * n, 0.0), b(n, 0.0), x(n, 0.0);
    for (int i = 0; i < n; i++)
        for (int j = i; j < n; j++) U[(size_t)i * n + j] = S[(size_t)i * n + j];
    int ok = 0;
    return ldlt_sparse_dense(n, U.data(), b.data(), x.data(), &ok, out, false);
}

}  // namespace orbgpu
