// loopcorrect.hip -- gfx950 LoopClosing map correction (reference src/LoopClosing.cc: CorrectLoop
// from CorrectedSim3[mpCurrentKF] = mg2oScw to the end of the CorrectedSim3 loop, and the tail of
// RunGlobalBundleAdjustment), driven by the Map handle's relation (map.hpp: MapView).
//
//   k_lc_sim3     one thread per listed keyframe: NonCorrectedSim3, CorrectedSim3 and its inverse,
//                 the SetPose argument [R | t / s] and its camera centre, all from the old poses
//   k_lc_claim    one thread per (listed keyframe, slot): atomicMin of the processing index per
//                 point, the first-occurrence idiom of k_map_pt_min (an integer minimum: order-free)
//   k_lc_points   one thread per (listed keyframe, slot); the thread whose keyframe won the claim
//                 corrects the point and runs UpdateNormalAndDepth.  The observers are taken in
//                 ascending keyframe id by repeated selection of the next larger id straight from
//                 the handle's unordered cell list: nothing is stored or sorted, at n^2 reads of
//                 cached words for n observers.  Map points carry a handful to a few tens of
//                 observers; there is no one-wave-per-point path for longer lists.
//   k_lc_pose     Tcw of the listed keyframes, after the points have read the old poses
//   k_gba_level   one dependent step of the spanning-tree propagation: one thread per child
//   k_gba_points  one thread per map point
//   k_gba_finish  one thread per keyframe row: TcwBefGBA = Tcw, Tcw = TcwGBA where reached
//
// Every float result is one IEEE operation sequence in a fixed order (no float atomics); the
// integer atomics form a minimum and, once per workgroup, two counts.
#include "loopcorrect.hpp"
#include "orb_common.hpp"
#include "sim3_math.hpp"

namespace orbgpu {

namespace {

constexpr int LT = 256;

__device__ __forceinline__ double norm3_d(const float (&v)[3]) {
    return sqrt(((double)v[0] * v[0] + (double)v[1] * v[1]) + (double)v[2] * v[2]);
}

// cv::gemm of two 4 x 4 float matrices: the sum over k ascending in double, one rounding
__device__ __forceinline__ void gemm4(const float* A, const float* B, float* o) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++)
            o[r * 4 + c] = (float)((((double)A[r * 4] * B[c] + (double)A[r * 4 + 1] * B[4 + c]) +
                                    (double)A[r * 4 + 2] * B[8 + c]) +
                                   (double)A[r * 4 + 3] * B[12 + c]);
}

// KeyFrame::SetPose: Ow = -Rwc * tcw (gemm with alpha -1)
__device__ __forceinline__ void centre_of(const float* T, float* Ow) {
#pragma unroll
    for (int r = 0; r < 3; r++)
        Ow[r] = (float)((((double)T[r] * T[3] + (double)T[4 + r] * T[7]) + (double)T[8 + r] * T[11]) * -1.0);
}

// Twc = [Rwc | Ow; 0 0 0 1]
__device__ __forceinline__ void twc_of(const float* T, float* W) {
    float Ow[3];
    centre_of(T, Ow);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) W[r * 4 + c] = T[c * 4 + r];
        W[r * 4 + 3] = Ow[r];
    }
    W[12] = W[13] = W[14] = 0.f;
    W[15] = 1.f;
}

// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)
__device__ __forceinline__ void sim3_of_pose(const float* T, Sim3d& S) {
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[r * 3 + c] = (double)T[r * 4 + c];
        S.t[r] = (double)T[r * 4 + 3];
    }
    quat_from_R(R, S.q);
    S.s = 1.0;
}

__global__ void __launch_bounds__(LT) k_lc_sim3(LoopCorrectDev D) {
    const int j = blockIdx.x * LT + threadIdx.x;
    if (j >= D.nkf) return;
    const int id = D.kf_id[j];
    D.proc[id] = j;
    float Ti[16];
    for (int k = 0; k < 16; k++) Ti[k] = D.Tcw[16 * (size_t)id + k];
    Sim3d non, cor;
    sim3_of_pose(Ti, non);
    const Sim3d Scw = *(const Sim3d*)D.Scw;
    if (j == D.cur) {
        cor = Scw;
    } else {
        float Tc[16], Twc[16], Tic[16];
        for (int k = 0; k < 16; k++) Tc[k] = D.Tcw[16 * (size_t)D.kf_id[D.cur] + k];
        twc_of(Tc, Twc);
        gemm4(Ti, Twc, Tic);
        Sim3d Sic;
        sim3_of_pose(Tic, Sic);
        sim3_mul(Sic, Scw, cor);
    }
    Sim3d inv;
    sim3_inverse(cor, inv);
    ((Sim3d*)D.noncorr)[j] = non;
    ((Sim3d*)D.corr)[j] = cor;
    ((Sim3d*)D.corr_inv)[j] = inv;
    // correctedTiw = [R | t * (1 / s)], as k_ess_finish
    double R[9];
    quat_to_R(cor.q, R);
    float N[16];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) N[r * 4 + c] = (float)R[r * 3 + c];
        N[r * 4 + 3] = (float)(cor.t[r] * (1. / cor.s));
    }
    N[12] = N[13] = N[14] = 0.f;
    N[15] = 1.f;
    for (int k = 0; k < 16; k++) D.newT[16 * (size_t)j + k] = N[k];
    float Ow[3];
    centre_of(N, Ow);
    for (int r = 0; r < 3; r++) D.newOw[3 * (size_t)j + r] = Ow[r];
}

__global__ void __launch_bounds__(LT) k_lc_claim(LoopCorrectDev D) {
    const int j = blockIdx.y;
    const MapSlotDev S = D.V.slots[D.kf_slot[j]];
    const int i = blockIdx.x * LT + threadIdx.x;
    if (i >= S.n) return;
    const int p = D.V.mp[S.off + i];
    if (p < 0 || p >= D.n_pt_rows) return;
    if (D.bad && D.bad[p]) return;
    atomicMin(&D.claim[p], j);
}

// the camera centre the reference sees for keyframe `id` while keyframe j corrects its points
__device__ __forceinline__ void centre_seen(const LoopCorrectDev& D, int id, int j, float* Ow) {
    const int pj = D.proc[id];
    if (pj >= 0 && pj < j) {
        for (int r = 0; r < 3; r++) Ow[r] = D.newOw[3 * (size_t)pj + r];
    } else {
        centre_of(D.Tcw + 16 * (size_t)id, Ow);
    }
}

// Slot i of listed keyframe j.  -> 0: not this keyframe's point to correct, 1: corrected, 2: corrected
// and left without UpdateNormalAndDepth for want of its reference keyframe
__device__ __forceinline__ int correct_slot(const LoopCorrectDev& D, int j, const MapSlotDev& S, int i) {
    if (i >= S.n) return 0;
    const int p = D.V.mp[S.off + i];
    if (p < 0 || p >= D.n_pt_rows) return 0;
    if (D.claim[p] != j) return 0;        // bad points were never claimed
    D.corrected_ref[p] = D.kf_id[j];
    // pos = correctedSwi.map(Siw.map(P3Dw))
    const double X0[3] = {(double)D.pos[3 * (size_t)p], (double)D.pos[3 * (size_t)p + 1], (double)D.pos[3 * (size_t)p + 2]};
    double c[3], w[3];
    sim3_map(((const Sim3d*)D.noncorr)[j], X0, c);
    sim3_map(((const Sim3d*)D.corr_inv)[j], c, w);
    const float X[3] = {(float)w[0], (float)w[1], (float)w[2]};
    for (int r = 0; r < 3; r++) D.pos[3 * (size_t)p + r] = X[r];
    // MapPoint::UpdateNormalAndDepth
    if (p >= D.V.npts) return 1;
    const int o0 = D.V.pt_start[p], o1 = D.V.pt_start[p + 1];
    if (o1 <= o0) return 1;
    const int ref = D.ref_kf[p];
    int ref_oct = -1;
    if (ref >= 0)
        for (int o = o0; o < o1; o++) {
            const uint32_t cell = D.V.pt_obs[o];
            const MapSlotDev K = D.V.slots[cell / kMapMaxRow];
            if (K.id == ref) ref_oct = D.V.oct[K.off + (int)(cell % kMapMaxRow)];
        }
    if (ref_oct < 0 || ref_oct >= D.nlevels) return 2;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int last = -1;
    for (int k = o0; k < o1; k++) {
        int next = 0x7fffffff;            // the smallest observer id above `last`
        for (int o = o0; o < o1; o++) {
            const int id = D.V.slots[D.V.pt_obs[o] / kMapMaxRow].id;
            if (id > last && id < next) next = id;
        }
        if (next == 0x7fffffff) break;    // a keyframe observes a point once: not reached
        last = next;
        float O[3];
        centre_seen(D, next, j, O);
        const float v[3] = {X[0] - O[0], X[1] - O[1], X[2] - O[2]};
        const float inv = (float)(1.0 / norm3_d(v));
#pragma unroll
        for (int r = 0; r < 3; r++) acc[r] = acc[r] + v[r] * inv;
    }
    const float invn = (float)(1.0 / (double)(o1 - o0));
#pragma unroll
    for (int r = 0; r < 3; r++) D.normal[3 * (size_t)p + r] = acc[r] * invn;
    float RO[3];
    centre_seen(D, ref, j, RO);
    const float PC[3] = {X[0] - RO[0], X[1] - RO[1], X[2] - RO[2]};
    const float dist = (float)norm3_d(PC);
    const float mx = dist * D.scale[ref_oct];
    D.max_dist[p] = mx;
    D.min_dist[p] = mx / D.scale[D.nlevels - 1];
    return 1;
}

// the two counts: one integer atomic per workgroup and count
__device__ __forceinline__ void count_block(int32_t* counts, bool a, bool b) {
    const int na = __syncthreads_count(a), nb = __syncthreads_count(b);
    if (threadIdx.x == 0) {
        if (na) atomicAdd(&counts[0], na);
        if (nb) atomicAdd(&counts[1], nb);
    }
}

__global__ void __launch_bounds__(LT) k_lc_points(LoopCorrectDev D) {
    const int j = blockIdx.y;
    const MapSlotDev S = D.V.slots[D.kf_slot[j]];
    const int kind = correct_slot(D, j, S, blockIdx.x * LT + threadIdx.x);
    count_block(D.counts, kind != 0, kind == 2);
}

__global__ void __launch_bounds__(LT) k_lc_pose(LoopCorrectDev D) {
    const int t = blockIdx.x * LT + threadIdx.x;
    if (t >= D.nkf * 16) return;
    D.Tcw[16 * (size_t)D.kf_id[t >> 4] + (t & 15)] = D.newT[t];
}

__global__ void __launch_bounds__(LT) k_gba_level(GbaApplyDev D, int lo, int hi) {
    const int t = lo + blockIdx.x * LT + threadIdx.x;
    if (t >= hi) return;
    const int child = D.pair[2 * (size_t)t], parent = D.pair[2 * (size_t)t + 1];
    float Tc[16], Tp[16], G[16], Twc[16], Tcp[16], out[16];
    for (int k = 0; k < 16; k++) {
        Tc[k] = D.Tcw[16 * (size_t)child + k];
        Tp[k] = D.Tcw[16 * (size_t)parent + k];
        G[k] = D.TcwGBA[16 * (size_t)parent + k];
    }
    twc_of(Tp, Twc);
    gemm4(Tc, Twc, Tcp);      // Tchildc = pChild->GetPose() * Twc
    gemm4(Tcp, G, out);       // pChild->mTcwGBA = Tchildc * pKF->mTcwGBA
    for (int k = 0; k < 16; k++) D.TcwGBA[16 * (size_t)child + k] = out[k];
}

// -> 0: untouched, 1: pos = posGBA, 2: re-expressed through the reference keyframe
__device__ __forceinline__ int gba_point(const GbaApplyDev& D, int p) {
    if (p >= D.n_pt_rows) return 0;
    if (D.bad && D.bad[p]) return 0;
    if (D.mp_in_gba[p]) {
        for (int r = 0; r < 3; r++) D.pos[3 * (size_t)p + r] = D.posGBA[3 * (size_t)p + r];
        return 1;
    }
    const int ref = D.ref_kf[p];
    if (ref < 0 || ref >= D.n_kf_rows || !D.reached[ref]) return 0;
    const float* B = D.Tcw + 16 * (size_t)ref;       // mTcwBefGBA: Tcw is rewritten after this kernel
    const float* G = D.TcwGBA + 16 * (size_t)ref;
    const float X[3] = {D.pos[3 * (size_t)p], D.pos[3 * (size_t)p + 1], D.pos[3 * (size_t)p + 2]};
    float Xc[3], Ow[3];
    for (int r = 0; r < 3; r++)
        Xc[r] = (float)((((double)B[r * 4] * X[0] + (double)B[r * 4 + 1] * X[1]) + (double)B[r * 4 + 2] * X[2]) +
                        (double)B[r * 4 + 3]);
    centre_of(G, Ow);
    for (int r = 0; r < 3; r++)
        D.pos[3 * (size_t)p + r] =
            (float)((((double)G[r] * Xc[0] + (double)G[4 + r] * Xc[1]) + (double)G[8 + r] * Xc[2]) + (double)Ow[r]);
    return 2;
}

__global__ void __launch_bounds__(LT) k_gba_points(GbaApplyDev D) {
    const int kind = gba_point(D, blockIdx.x * LT + threadIdx.x);
    count_block(D.counts, kind == 1, kind == 2);
}

__global__ void __launch_bounds__(LT) k_gba_finish(GbaApplyDev D) {
    const int t = blockIdx.x * LT + threadIdx.x;
    if (t >= D.n_kf_rows * 16) return;
    if (!D.reached[t >> 4]) return;
    if (D.TcwBef) D.TcwBef[t] = D.Tcw[t];
    D.Tcw[t] = D.TcwGBA[t];
}

unsigned blocks(long long n) { return (unsigned)((n + LT - 1) / LT); }

}  // namespace

int loop_correct_launch(const LoopCorrectDev& D, int max_row, hipStream_t s) {
    if (D.nkf <= 0) return 0;
    hipLaunchKernelGGL(k_lc_sim3, dim3(blocks(D.nkf)), dim3(LT), 0, s, D);
    if (max_row > 0) {
        const dim3 grid(blocks(max_row), (unsigned)D.nkf);
        hipLaunchKernelGGL(k_lc_claim, grid, dim3(LT), 0, s, D);
        hipLaunchKernelGGL(k_lc_points, grid, dim3(LT), 0, s, D);
    }
    hipLaunchKernelGGL(k_lc_pose, dim3(blocks((long long)D.nkf * 16)), dim3(LT), 0, s, D);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

int gba_apply_launch(const GbaApplyDev& D, int nlevels, const int* level_off, hipStream_t s) {
    for (int l = 0; l < nlevels; l++) {
        const int lo = level_off[l], hi = level_off[l + 1];
        if (hi > lo) hipLaunchKernelGGL(k_gba_level, dim3(blocks(hi - lo)), dim3(LT), 0, s, D, lo, hi);
    }
    if (D.n_pt_rows > 0) hipLaunchKernelGGL(k_gba_points, dim3(blocks(D.n_pt_rows)), dim3(LT), 0, s, D);
    hipLaunchKernelGGL(k_gba_finish, dim3(blocks((long long)D.n_kf_rows * 16)), dim3(LT), 0, s, D);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace orbgpu
