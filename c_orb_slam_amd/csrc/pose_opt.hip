// pose_opt.hip -- gfx950 Optimizer::PoseOptimization (PoseEngine, declared in ba.hpp): the edge
// pack kernel (k_pose_pack), the persistent per-frame optimiser (k_pose_opt) and their host
// launches; the test-only kernels k_unit_se3 and k_pose_stage (orbgpu_unit_se3,
// orbgpu_unit_pose_stage), which run the same device functions one stage at a time.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "ba.hpp"
#include "ba_math.hpp"
#include "orb_common.hpp"

namespace orbgpu {

// ---------------------------------------------------------------- PoseOptimization
// Optimizer::PoseOptimization (Optimizer.cc:239-451): one SE3 vertex with unary
// EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose edges
// (types_six_dof_expmap.cpp:266-364), solved by LinearSolverDense (Eigen LDLT with diagonal
// pivoting).  The whole call -- 4 rounds of optimize(10), each restarted from mTcw, with the
// outlier classification after every round -- is ONE persistent workgroup per frame (a batch
// of frames is one launch).  Per LM iteration: one fused pass over the active edges (errors,
// robust chi2 and the 27 terms of the 6x6 system, canonical 64-tree sums of oracle/ba.c),
// then per trial the register-resident pivoted LDL^T + SE3 update on thread 0 and one error
// pass.  Edges are 32 B (the reference's float inputs; converted to double on load) and each
// wave prefetches its next chunk's edges while it computes the current one.
struct PoseEdgeDev {
    float Xw[3], obs[3];   // GetWorldPos(); kpUn.pt.x, .y, mvuRight
    float info;            // mvInvLevelSigma2[octave]
    int meta;              // bit 31: stereo edge; bits 0-30: keypoint index
};

struct PoseProbDev {
    int ne, e0;            // edges E[e0 .. e0+ne)
    int nbad, N;           // out: nBad of the last round (-1: < 3 correspondences)
    Se3 T0;                // Converter::toSE3Quat(pFrame->mTcw)
    Se3 T;                 // out
    double fx, fy, cx, cy, bf;
    // device mode: the frame's arrays in HBM (edges are built by k_pose_pack, results
    // written back by k_pose_opt's epilogue); null in host mode
    const float* Tcw;
    const uint8_t* has_mp;
    const float* Xw;
    const float* obs;
    const float* inv_sigma2;
    float* Tcw_out;
    uint8_t* outlier;
    // frame mode (pose_frame): gathered by k_pose_pack instead of the packed arrays above
    const int* mpidx;          // mvpMapPoints as indices (-1 NULL)
    const float* mp_pos;       // map point rows (GetWorldPos)
    const float* keys;         // mvKeysUn, 7 words per cv::KeyPoint (x y size angle response octave class_id)
    const float* uR;           // mvuRight
    const float* isig_tab;     // mvInvLevelSigma2
    int nlev;
    int* ninl;                 // optional device out: inliers (ne - nBad), 0 below 3 edges, -1 over capacity
};

// one edge in double (the g2o edge's _measurement / information / Huber delta)
struct PoseEdgeD {
    double X[3], obs[3], info, delta, dsqr;
    bool stereo;
};

__device__ __forceinline__ PoseEdgeD pose_edge_load(const PoseEdgeDev* E, int i, double dM, double dS) {
    const uint4* p = reinterpret_cast<const uint4*>(E + i);
    const uint4 a = p[0], b = p[1];
    PoseEdgeD e;
    e.X[0] = (double)__uint_as_float(a.x);
    e.X[1] = (double)__uint_as_float(a.y);
    e.X[2] = (double)__uint_as_float(a.z);
    e.obs[0] = (double)__uint_as_float(a.w);
    e.obs[1] = (double)__uint_as_float(b.x);
    e.obs[2] = (double)__uint_as_float(b.y);
    e.info = (double)__uint_as_float(b.z);
    e.stereo = (b.w >> 31) != 0;
    e.delta = e.stereo ? dS : dM;   // RobustKernelHuber delta = sqrt(chi2 threshold) as float
    e.dsqr = e.delta * e.delta;
    return e;
}

// the error at camera point p (dz: the shared divisions by p[2])
__device__ __forceinline__ void pose_err_p(const PoseEdgeD& e, const double* p, const SharedDiv& dz,
                                           const PoseProbDev& P, double* err) {
    if (!e.stereo) {
        const double px = dz.div(p[0]), py = dz.div(p[1]);
        err[0] = e.obs[0] - (px * P.fx + P.cx);
        err[1] = e.obs[1] - (py * P.fy + P.cy);
        err[2] = 0;
    } else {
        const float invz = (float)dz.div(1.0);
        const double u = (p[0] * (double)invz) * P.fx + P.cx;
        const double v = (p[1] * (double)invz) * P.fy + P.cy;
        err[0] = e.obs[0] - u;
        err[1] = e.obs[1] - v;
        err[2] = e.obs[2] - (u - P.bf * (double)invz);
    }
}

__device__ __forceinline__ void pose_err(const PoseEdgeD& e, const Se3& T, const PoseProbDev& P, double* err) {
    double p[3];
    se3_map(T, e.X, p);
    pose_err_p(e, p, SharedDiv(p[2]), P, err);
}

__device__ __forceinline__ double pose_chi2(const PoseEdgeD& e, const double* err) {
    double s = err[0] * (e.info * err[0]);
    s += err[1] * (e.info * err[1]);
    if (e.stereo) s += err[2] * (e.info * err[2]);
    return s;
}

__device__ __forceinline__ double pose_rho0(const PoseEdgeD& e, double c, bool robust) {
    if (!robust || c <= e.dsqr) return c;
    const double sq = sqrt(c);
    return (2 * sq) * e.delta - e.dsqr;
}


// J, robust weight and the 28 entries (robust chi2, J^T W J upper triangle, -J^T W e) of one edge
// at pose X, into v[0..28); rb: the edge's robust kernel is set.  J (3 x 6, row-major) and the
// error e3 are the caller's, so that the stage kernel (k_pose_stage) can report them.
__device__ __forceinline__ void pose_sys_terms_je(const PoseEdgeD& e, bool rb, const Se3& X, const PoseProbDev& P,
                                                  double* v, double* J, double* e3) {
    double p[3];
    se3_map(X, e.X, p);
    const SharedDiv dz(p[2]);
    pose_err_p(e, p, dz, P, e3);
    const double c = pose_chi2(e, e3);
    v[0] = pose_rho0(e, c, rb);
    const double x = p[0], y = p[1], invz = dz.div(1.0), invz_2 = invz * invz;
    J[0] = ((x * y) * invz_2) * P.fx;
    J[1] = (-(1 + ((x * x) * invz_2))) * P.fx;
    J[2] = (y * invz) * P.fx;
    J[3] = (-invz) * P.fx;
    J[4] = 0;
    J[5] = (x * invz_2) * P.fx;
    J[6] = (1 + ((y * y) * invz_2)) * P.fy;
    J[7] = (((-x) * y) * invz_2) * P.fy;
    J[8] = ((-x) * invz) * P.fy;
    J[9] = 0;
    J[10] = (-invz) * P.fy;
    J[11] = (y * invz_2) * P.fy;
    J[12] = J[0] - ((P.bf * y) * invz_2);
    J[13] = J[1] + ((P.bf * x) * invz_2);
    J[14] = J[2];
    J[15] = J[3];
    J[16] = 0;
    J[17] = J[5] - (P.bf * invz_2);
    // monocular edges: a zero third Jacobian row (and err[2] = 0) makes every
    // third term +-0, an exact identity on the two-term partial sums (which
    // start from +0 + t0 and so are never -0): the sums run branch-free
#pragma unroll
    for (int j = 12; j < 18; j++) J[j] = e.stereo ? J[j] : 0.0;
    double r1 = 1.;
    if (rb && !(c <= e.dsqr)) r1 = e.delta / sqrt(c);
    const double wgt = rb ? r1 * e.info : e.info;
    double omr[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
        omr[kk] = -(e.info * e3[kk]);
        if (rb) omr[kk] *= r1;
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double sb = 0;
#pragma unroll
        for (int kk = 0; kk < 3; kk++) sb += J[kk * 6 + r] * omr[kk];
        v[22 + r] = sb;
#pragma unroll
        for (int cc = r; cc < 6; cc++) {
            double hh = 0;
#pragma unroll
            for (int kk = 0; kk < 3; kk++) hh += (J[kk * 6 + r] * wgt) * J[kk * 6 + cc];
            v[1 + r * 6 - (r * (r - 1)) / 2 + (cc - r)] = hh;
        }
    }
}
__device__ __forceinline__ void pose_sys_terms(const PoseEdgeD& e, bool rb, const Se3& X, const PoseProbDev& P,
                                               double* v) {
    double J[18], e3[3];
    pose_sys_terms_je(e, rb, X, P, v, J, e3);
}


constexpr int kPoseMaxEdges = 8192;
// two waves per SIMD (512 threads): half the chunks per wave in every edge pass (the same
// canonical sums: bit-identical).  Measured in the pipeline beside the extraction grids too:
// 28.8 k vs 28.1 k frames/s for the one-wave-per-SIMD instance (256 threads) at B = 64, so
// every batch takes it; ORBGPU_POSE_WIDE_MAX = F keeps it for batches of at most F frames only
constexpr int kPoseThreads = 256, kPoseThreadsWide = 512;
static int pose_wide_max() {
    static const int v = [] {
        const char* e = getenv("ORBGPU_POSE_WIDE_MAX");
        return e ? atoi(e) : (1 << 30);
    }();
    return v;
}

// Opt-in (ORBGPU_POSE_LDS_KB=n): reserve n KiB of LDS per pose workgroup in the chained batch
// launch, so that the extraction grids' LDS-staged kernels cannot share the CUs the pose
// workgroups run on (dynamic bytes added on top of the kernel's static LDS)
static size_t pose_lds_pad(const void* fn) {
    static const int kb = [] {
        const char* e = getenv("ORBGPU_POSE_LDS_KB");
        return e ? atoi(e) : 0;
    }();
    if (kb <= 0) return 0;
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, fn) != hipSuccess) return 0;
    const size_t want = (size_t)std::min(kb, 160) * 1024;
    return want > a.sharedSizeBytes ? want - a.sharedSizeBytes : 0;
}

// Canonical totals (ora_csum level 2) of the m chunk trees cs[q][0..m) of K sums, by wave 0:
// lane c holds chunk c and the K trees run packed (the same pairing as local_csum_inplace).
// K = 28 is split over waves 0-3, 7 trees each (every value's packed tree is the canonical one
// whatever the packing width, so the split changes no bit; wave 0 alone was a serial segment of
// every LM trial).
template <int K>
__device__ __forceinline__ void pose_chunk_totals(double (*cs)[kPoseMaxEdges / 64], int m, double* res) {
    constexpr int KW = K == 28 ? 7 : K;
    const int w = threadIdx.x >> 6;
    if (w >= K / KW) return;
    const int lane = threadIdx.x & 63, q0 = w * KW;
    if (m <= 1) {
        if (lane < KW) res[q0 + lane] = m == 1 ? cs[q0 + lane][0] : 0.0;
    } else if (m <= 64) {
        double v[KW];
#pragma unroll
        for (int q = 0; q < KW; q++) v[q] = lane < m ? cs[q0 + q][lane] : 0.0;
        const double t = packed_trees<KW>(v);
        const int q = bitrev6(lane);
        if (q < KW) res[q0 + q] = t;
    } else if (lane < KW) {
        res[q0 + lane] = local_csum_inplace(cs[q0 + lane], m);
    }
}

// Block-wide canonical sums (ora_csum) of K per-active-edge values: wave w owns chunks
// c = w, w + nw, ... of 64 active edges; the edge of chunk c + nw is loaded while chunk c is
// computed.  f(e, i, out[K]) evaluates active edge i (edge e loaded).  Chunk trees go to
// cs[q][c]; thread q < K finishes entry q.
template <int K, class F, class Post>
// post: run by thread 0 right after its own totals (res[0] among them) and before the closing
// barrier, i.e. beside the other waves' totals
__device__ __forceinline__ void pose_pass_post(F f, int nA, const uint16_t* aE, const PoseEdgeDev* E, double dM,
                                               double dS, double (*cs)[kPoseMaxEdges / 64], double* res,
                                               const PoseEdgeD& mine, int mineIdx, Post post) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int m = (nA + 63) >> 6;
    // chunk c = w is active edge tid: this thread's for the whole round, kept in registers
    // (loaded once per round); later chunks are loaded one ahead.  One code path for every
    // chunk count keeps a single inlined copy of f per call site (instruction-cache footprint)
    int c = w;
    int a = threadIdx.x;
    int i = mineIdx;
    PoseEdgeD e = mine;
    while (c < m) {
        const int cn = c + nw, an = cn * 64 + lane;
        int in = 0;
        PoseEdgeD en = e;
        if (cn < m) {   // prefetch the next chunk's edge
            in = an < nA ? aE[an] : 0;
            en = pose_edge_load(E, in, dM, dS);
        }
        double v[K];
        if (a < nA) f(e, i, v);
        else
#pragma unroll
            for (int q = 0; q < K; q++) v[q] = 0.0;
        if (nA == 1) {   // ora_csum keeps a single term untouched
            if (lane == 0)
#pragma unroll
                for (int q = 0; q < K; q++) cs[q][0] = v[q];
        } else {
            const double t = packed_trees<K>(v);
            const int q = bitrev6(lane);
            if (q < K) cs[q][c] = t;
        }
        c = cn;
        a = an;
        i = in;
        e = en;
    }
    __syncthreads();
    pose_chunk_totals<K>(cs, nA > 0 ? m : 0, res);
    if (threadIdx.x == 0) post();
    __syncthreads();
}
template <int K, class F>
__device__ __forceinline__ void pose_pass(F f, int nA, const uint16_t* aE, const PoseEdgeDev* E, double dM, double dS,
                                          double (*cs)[kPoseMaxEdges / 64], double* res, const PoseEdgeD& mine,
                                          int mineIdx) {
    pose_pass_post<K>(f, nA, aE, E, dM, dS, cs, res, mine, mineIdx, [] {});
}


// ---- wave-level dense solve of the pose system ---------------------------------------
__device__ __forceinline__ double lane_bcast(double v, int l) {
    const unsigned long long u = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)(u & 0xffffffffu), l);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
// N independent IEEE divisions num[j] / den[j] as ONE lane-parallel division (lane j), results
// broadcast to every lane.  The whole wave must be active and hold the same operands.
template <int N>
__device__ __forceinline__ void lane_div(const double* num, const double* den, double* out) {
    const int lane = threadIdx.x & 63;
    double a = num[0], b = den[0];
#pragma unroll
    for (int j = 1; j < N; j++) {
        // opaque operands: a select chain over an array indexed by the lane otherwise becomes
        // a scratch-memory lookup
        double nj = num[j], dj = den[j];
        asm volatile("" : "+v"(nj), "+v"(dj));
        a = lane == j ? nj : a;
        b = lane == j ? dj : b;
    }
    const double q = a / b;
#pragma unroll
    for (int j = 0; j < N; j++) out[j] = lane_bcast(q, j);
}

// LinearSolverDense (Eigen LDLT with diagonal pivoting) of (H + lambda I) x = b, H the packed
// upper triangle Hs[21], run redundantly by a whole wave: the same IEEE operations as
// ldlt_pivot6.  Left-looking LDLT never touches a diagonal entry before its own step, so the
// pivot sequence is a function of |diag(H) + lambda| alone: it is fixed first, the
// factorisation then runs unpivoted on P A P^T with static register indices, and the row
// divisions of a step (and the 6 of the solve) are one lane-parallel division each.
__device__ __forceinline__ bool pose_solve_w(const double* Hs, const double* bs, double lambda, double* x) {
    // With distinct |pivots| the sequence is the descending order of |diag| (ties or NaN take
    // the reference routine: its tie-break follows the swap history).  Ranks instead of swaps
    // keep every index static (no scratch).
    double dv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) dv[i] = fabs(Hs[DIAG21[i]] + lambda);
    bool distinct = true;
    int rank[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        int r = 0;
        distinct = distinct && dv[j] == dv[j];
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (i != j) {
                r += dv[i] > dv[j] ? 1 : 0;
                distinct = distinct && dv[i] != dv[j];
            }
        rank[j] = r;
    }
    int ord[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        int o = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) o = rank[j] == r ? j : o;
        ord[r] = o;
    }
    double A[36];   // lower triangle of P (H + lambda I) P^T
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) {
            const int a = min(ord[r], ord[c]), b = max(ord[r], ord[c]);
            double h = Hs[a * 6 - (a * (a - 1)) / 2 + (b - a)];
            if (r == c) h += lambda;
            A[r * 6 + c] = h;
        }
    if (!distinct || !(fabs(A[0]) > 0.0)) {   // ties / NaN, or the reference's zero-pivot stop
        double Hd[36], bb[6];
#pragma unroll
        for (int r = 0, q = 0; r < 6; r++)
#pragma unroll
            for (int cc = r; cc < 6; cc++, q++) {
                double h = Hs[q];
                if (cc == r) h += lambda;
                Hd[r * 6 + cc] = h;
                Hd[cc * 6 + r] = h;
            }
#pragma unroll
        for (int j = 0; j < 6; j++) bb[j] = bs[j];
        return ldlt_pivot6(Hd, bb, x);
    }
    int sign = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (k > 0) {
            double tmp[6];
#pragma unroll
            for (int j = 0; j < k; j++) tmp[j] = A[j * 6 + j] * A[k * 6 + j];
            double s = 0;
#pragma unroll
            for (int j = 0; j < k; j++) s += A[k * 6 + j] * tmp[j];
            A[k * 6 + k] -= s;
#pragma unroll
            for (int i = k + 1; i < 6; i++) {
                double t = 0;
#pragma unroll
                for (int j = 0; j < k; j++) t += A[i * 6 + j] * tmp[j];
                A[i * 6 + k] -= t;
            }
        }
        const double akk = A[k * 6 + k];
        if (k < 5 && fabs(akk) > 0.0) {
            double num[5], den[5], q[5];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                num[j] = k + 1 + j < 6 ? A[(k + 1 + j) * 6 + k] : 1.0;
                den[j] = akk;
            }
            lane_div<5>(num, den, q);
#pragma unroll
            for (int i = k + 1; i < 6; i++) A[i * 6 + k] = q[i - k - 1];
        }
        if (sign == 1) {
            if (akk < 0) sign = 3;
        } else if (sign == 2) {
            if (akk > 0) sign = 3;
        } else if (sign == 0) {
            if (akk > 0) sign = 1;
            else if (akk < 0) sign = 2;
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] = bs[ord[i]];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < i; j++) y[i] -= A[i * 6 + j] * y[j];
    {
        double den[6], q[6];
#pragma unroll
        for (int i = 0; i < 6; i++) den[i] = A[i * 6 + i];
        lane_div<6>(y, den, q);
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] = fabs(A[i * 6 + i]) > DBL_MIN ? q[i] : 0.0;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--)
#pragma unroll
        for (int j = 5; j > i; j--) y[i] -= A[j * 6 + i] * y[j];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double v = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++)
            if (ord[p] == j) v = y[p];
        x[j] = v;
    }
    return true;
}

// The same solve with lane r holding row r of P (H + lambda I) P^T (lanes >= 6 shadow row 5):
// every IEEE operation of pose_solve_w, each row's in the lane that owns it, so a step's row
// updates and divisions are one lane-parallel instruction each and only the pivot and the
// finished y_j travel between lanes; the backward sweep reads the columns of L through scr
// (36 doubles of this wave's LDS).  x is returned in every lane.
__device__ __forceinline__ bool pose_solve_l(const double* Hs, const double* bs, double lambda, double* x,
                                             double* scr) {
    double dv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) dv[i] = fabs(Hs[DIAG21[i]] + lambda);
    bool distinct = true;
    int rank[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        int r = 0;
        distinct = distinct && dv[j] == dv[j];
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (i != j) {
                r += dv[i] > dv[j] ? 1 : 0;
                distinct = distinct && dv[i] != dv[j];
            }
        rank[j] = r;
    }
    int ord[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        int o = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) o = rank[j] == r ? j : o;
        ord[r] = o;
    }
    const double a00 = Hs[DIAG21[ord[0]]] + lambda;
    if (!distinct || !(fabs(a00) > 0.0)) {   // ties / NaN, or the reference's zero-pivot stop
        double Hd[36], bb[6];
#pragma unroll
        for (int r = 0, q = 0; r < 6; r++)
#pragma unroll
            for (int cc = r; cc < 6; cc++, q++) {
                double h = Hs[q];
                if (cc == r) h += lambda;
                Hd[r * 6 + cc] = h;
                Hd[cc * 6 + r] = h;
            }
#pragma unroll
        for (int j = 0; j < 6; j++) bb[j] = bs[j];
        return ldlt_pivot6(Hd, bb, x);
    }
    const int lane = threadIdx.x & 63, row = lane < 6 ? lane : 5;
    int orow = ord[0];
#pragma unroll
    for (int p = 1; p < 6; p++) orow = row == p ? ord[p] : orow;
    double a[6];   // row `row` of P (H + lambda I) P^T, lower part used
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const int i0 = min(orow, ord[c]), i1 = max(orow, ord[c]);
        double h = Hs[i0 * 6 - (i0 * (i0 - 1)) / 2 + (i1 - i0)];
        if (row == c) h += lambda;
        a[c] = h;
    }
    // branch-free: the reference's sign state machine ends in 1 / 2 / 3 / 0 exactly when some /
    // only positive, only negative, both, no nonzero pivots were seen, so two flags replace it
    double d[6];
    bool anyNeg = false;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (k > 0) {
            double tmp[6];
#pragma unroll
            for (int j = 0; j < k; j++) tmp[j] = d[j] * lane_bcast(a[j], k);   // A[j][j] * A[k][j]
            double u = 0;
#pragma unroll
            for (int j = 0; j < k; j++) u += a[j] * tmp[j];
            const double ak = a[k] - u;
            a[k] = row >= k ? ak : a[k];
        }
        const double akk = lane_bcast(a[k], k);
        d[k] = akk;
        if (k < 5) {
            const double q = a[k] / akk;
            a[k] = (fabs(akk) > 0.0 && row > k) ? q : a[k];
        }
        anyNeg = anyNeg || akk < 0;
    }
    if (anyNeg) return false;
    double y = bs[orow];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const double yj = lane_bcast(y, j);
        const double v = y - a[j] * yj;
        y = row > j ? v : y;
    }
    double arr = a[0];
#pragma unroll
    for (int c = 1; c < 6; c++) arr = row == c ? a[c] : arr;   // own diagonal
    {
        const double q = y / arr;
        y = fabs(arr) > DBL_MIN ? q : 0.0;
    }
    // columns of L: lane r needs A[j][r], j > r
    if (lane < 6)
#pragma unroll
        for (int c = 0; c < 6; c++) scr[lane * 6 + c] = a[c];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    double col[6];
#pragma unroll
    for (int j = 0; j < 6; j++) col[j] = scr[j * 6 + row];
#pragma unroll
    for (int j = 5; j >= 1; j--) {
        const double xj = lane_bcast(y, j);
        const double v = y - col[j] * xj;
        y = row < j ? v : y;
    }
    double yb[6];
#pragma unroll
    for (int p = 0; p < 6; p++) yb[p] = lane_bcast(y, p);
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double v = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++)
            if (ord[p] == j) v = yb[p];
        x[j] = v;
    }
    return true;
}

// k_pose_stage's copy of k_pose_opt's compaction (integer code only; k_pose_opt keeps its own
// inline: calling this function there changed its register allocation): active edges (bit 0 of fl
// clear) in edge order into aE, their count into *nA; ends with a barrier
template <int NT>
__device__ __forceinline__ void pose_compact(const uint8_t* fl, int ne, uint16_t* aE, int* wsum, int* nA) {
    constexpr int kPosePer = kPoseMaxEdges / NT;
    const int tid = threadIdx.x;
    const int base = tid * kPosePer;
    int c = 0;
    for (int j = 0; j < kPosePer; j++) c += (base + j < ne && (fl[base + j] & 1) == 0) ? 1 : 0;
    int incl = c;   // inclusive scan within the wave
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if ((tid & 63) >= o) incl += t;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < (tid >> 6); w++) off += wsum[w];
    int pos = off + incl - c;
    for (int j = 0; j < kPosePer; j++)
        if (base + j < ne && (fl[base + j] & 1) == 0) aE[pos++] = (uint16_t)(base + j);
    if (tid == blockDim.x - 1) *nA = off + incl;
    __syncthreads();
}

template <int NT>
__global__ void __launch_bounds__(NT) k_pose_opt(PoseProbDev* probs, const PoseEdgeDev* __restrict__ Eall,
                                                 double* errAll, uint8_t* outlAll) {
    ORBGPU_LATENCY_WAVE();
    PoseProbDev& P = probs[blockIdx.x];
    const int ne = P.ne;
    const PoseEdgeDev* E = Eall + P.e0;
    (void)errAll;   // errors are recomputed at classification instead of kept per pass
    uint8_t* outl = outlAll + P.e0;
    // LDS kept near 53 KiB so three workgroups fit a CU next to the extraction kernels: edge
    // flags (bit 0: level 1 = inactive, bit 1: robust kernel set), active-edge list as u16
    __shared__ uint8_t fl[kPoseMaxEdges];
    __shared__ uint16_t aE[kPoseMaxEdges];
    __shared__ double cs[28][kPoseMaxEdges / 64];
    __shared__ double red[32];
    // speculative solves for 1..kPoseSpec consecutive rejections of a trial (waves 1..kPoseSpec)
    constexpr int kPoseSpec = 3;
    __shared__ Se3 T, Terr, Tbase, Tc[kPoseSpec + 1];   // Tc: the candidates of a round of trials
    __shared__ double xc[kPoseSpec + 1][6];
    __shared__ int okc[kPoseSpec + 1];
    __shared__ double scrSolve[kPoseSpec + 1][36];   // pose_solve_l's column exchange, one per solving wave
    __shared__ double xs[6], Hs[21], bs[6], sysN[28];
    __shared__ double lambda, ni, currentChi, iniChi;
    __shared__ int nA, nBadLM, qmax, again, term, nBad, haveSys, specPass, wsum[16];
    const int tid = threadIdx.x;
    const double dM = (double)(float)sqrt(5.991), dS = (double)(float)sqrt(7.815);
    if (ne < 0) {   // device mode: capacity exceeded (reported by the host)
        if (tid == 0 && P.ninl) *P.ninl = -1;
        return;
    }
    if (ne < 3) {
        if (tid == 0) {
            P.T = P.T0;
            P.nbad = -1;
            if (P.ninl) *P.ninl = 0;
        }
        if (P.Tcw_out) {
            if (tid < 16) P.Tcw_out[tid] = P.Tcw[tid];
            for (int i = tid; i < ne; i += blockDim.x) P.outlier[E[i].meta & 0x7fffffff] = 0;
            // Tcw_out may be pinned host memory read by a host that polls a later kernel's signal
            // word: write the pose back at system scope before this workgroup ends
            if (tid < 16) __threadfence_system();
        }
        return;
    }
    for (int i = tid; i < ne; i += blockDim.x) {
        fl[i] = 2;
        outl[i] = 0;
    }
    __syncthreads();
    const float chi2Mono = 5.991f, chi2Stereo = 7.815f;
    for (int it = 0; it < 4; it++) {
        if (tid == 0) {
            T = P.T0;   // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) every round
            for (int j = 0; j < 6; j++) xs[j] = 0.0;
        }
        // active edges (level 0) in edge order: block prefix over kPosePer edges per thread
        {
            constexpr int kPosePer = kPoseMaxEdges / NT;
            const int base = tid * kPosePer;
            int c = 0;
            for (int j = 0; j < kPosePer; j++) c += (base + j < ne && (fl[base + j] & 1) == 0) ? 1 : 0;
            int incl = c;   // inclusive scan within the wave
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if ((tid & 63) >= o) incl += t;
            }
            if ((tid & 63) == 63) wsum[tid >> 6] = incl;
            __syncthreads();
            int off = 0;
            for (int w = 0; w < (tid >> 6); w++) off += wsum[w];
            int pos = off + incl - c;
            for (int j = 0; j < kPosePer; j++)
                if (base + j < ne && (fl[base + j] & 1) == 0) aE[pos++] = (uint16_t)(base + j);
            if (tid == blockDim.x - 1) nA = off + incl;
            __syncthreads();
        }
        const int na = nA;
        const int myIdx = tid < na ? aE[tid] : 0;
        const PoseEdgeD myE = pose_edge_load(E, myIdx, dM, dS);
        if (na > 0) {   // optimize(10); without active edges the vertex is not optimised at all
            ORBGPU_PROF_START;
            // the 28 entries of active edge i at pose X (pose_sys_terms), into v[0..28)
            auto sys_terms = [&](const PoseEdgeD& e, int i, const Se3& X, double* v) {
                pose_sys_terms(e, (fl[i] & 2) != 0, X, P, v);
            };
            // One LM iteration is a system pass at T (skipped when the accepted trial of the
            // previous iteration already evaluated it) followed by trials; a trial is the solves
            // (waves 0..kPoseSpec) and ONE pass at candidate 0.  Both passes run through the same
            // call site (sysPhase picks the pose), and the four solves through one: a single
            // inlined copy of the 28-sum edge body keeps the LM loop's code within the
            // instruction cache the workgroup shares with its neighbours.
            if (tid == 0) haveSys = 0;
            __syncthreads();
            int kit = 0;            // LM iteration (uniform: every thread steps it alike)
            bool sysPhase = true;   // the next pass evaluates the system at T
            for (;;) {
                if (!sysPhase) {
                    ORBGPU_PROF_MARK(10);
                    // Trials, up to four per round: candidate 0 solves at the current lambda
                    // (wave 0) while waves 1..kPoseSpec solve the systems of 1..kPoseSpec
                    // consecutive rejections (lambda *= ni; ni *= 2, the same H, b and starting
                    // estimate).  The pass of the first trial computes the whole system at
                    // candidate 0 (its robust chi2 is entry 0), so an accepted first trial hands
                    // the next iteration its system; a rejected one is followed by ONE pass for
                    // the speculative candidates, whose trials are then replayed in the
                    // reference's order.
                    if (tid < 64 * (kPoseSpec + 1)) {
                        const int L = tid >> 6;   // 0: the current trial, L: L rejections ahead
                        double ls = lambda, ns = ni;
                        for (int j = 0; j < L; j++) {
                            ls *= ns;
                            ns *= 2;
                        }
                        double xn[6];
#ifndef ORBGPU_POSE_SOLVE_W
                        const bool ok = pose_solve_l(Hs, bs, ls, xn, scrSolve[L]);
#else
                        const bool ok = pose_solve_w(Hs, bs, ls, xn);
#endif
                        ORBGPU_PROF_MARK(5);
                        ORBGPU_PROF_COUNT(9);
                        // candidate 0 steps from xs when the solve fails (its trial is then
                        // rejected: tempChi = DBL_MAX); a failed speculative solve stays at Tbase
                        double xl[6];
#pragma unroll
                        for (int j = 0; j < 6; j++) xl[j] = (ok || L > 0) ? xn[j] : xs[j];
                        Se3 r = Tbase;
                        if (ok || L == 0) {
                            Se3 d;
                            se3_exp(xl, d);
                            se3_mul(d, Tbase, r);
                        }
                        if ((tid & 63) == 0) {
                            Tc[L] = r;
#pragma unroll
                            for (int j = 0; j < 6; j++) xc[L][j] = xl[j];
                            okc[L] = ok ? 1 : 0;
                        }
                    }
                    __syncthreads();
                    ORBGPU_PROF_MARK(2);
                } else {
                    ORBGPU_PROF_MARK(0);
                    ORBGPU_PROF_COUNT(8);
                }
                // one trial of the reference's loop (optimization_algorithm_levenberg.cpp:100-149)
                // at candidate j with robust chi2 tempChi; tid 0 only
                auto trial = [&](int j, double tempChi) {
                    if (!okc[j]) tempChi = DBL_MAX;
#pragma unroll
                    for (int q = 0; q < 6; q++) xs[q] = xc[j][q];
                    double rho = currentChi - tempChi;
                    double sv[6];
                    for (int q = 0; q < 6; q++) sv[q] = xs[q] * (lambda * xs[q] + bs[q]);
                    double scale = tree64_local([&](int q) { return sv[q]; }, 6);
                    scale += 1e-3;
                    rho /= scale;
                    Terr = Tc[j];   // the pose of the last computeActiveErrors
                    if (rho > 0 && isfinite(tempChi)) {
                        const double a3 = 2 * rho - 1;
                        double alpha = 1. - (a3 * a3) * a3;
                        alpha = fmin(alpha, 2. / 3.);
                        const double scaleFactor = fmax(1. / 3., alpha);
                        lambda *= scaleFactor;
                        ni = 2;
                        currentChi = tempChi;
                        T = Tc[j];
                        if (j == 0) haveSys = 1;   // red[0..28) is the system at the new estimate
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        T = Tbase;
                    }
                    qmax++;
                    again = (rho < 0 && qmax < 10) ? 1 : 0;
                    if (!again) {
                        if (qmax == 10 || rho == 0) {
                            term = 1;
                        } else {
                            if ((iniChi - currentChi) * 1e3 < iniChi) nBadLM++;
                            else nBadLM = 0;
                            term = nBadLM >= 3 ? 1 : 0;
                        }
                    }
                };
                // sysPhase: computeActiveErrors + activeRobustChi2 (entry 0) and buildSystem
                // (entries 1..27) at T; a trial: its robust chi2 at candidate 0 and, with it, the
                // system at that estimate (the next iteration's whenever the trial is accepted).
                // Canonical sums per entry.
                {   // a trial's decision runs on thread 0 as soon as its chi2 total (red[0]) is in,
                    // beside the other waves' totals (the pass reads no state the decision writes)
                    const Se3& X = sysPhase ? T : Tc[0];
                    pose_pass_post<28>([&](const PoseEdgeD& e, int i, double* v) { sys_terms(e, i, X, v); }, na, aE, E,
                                       dM, dS, cs, red, myE, myIdx, [&] {
                                           if (!sysPhase) {
                                               trial(0, red[0]);
                                               specPass = again && okc[1] ? 1 : 0;
                                           }
                                       });
                }
                if (sysPhase) {
                    ORBGPU_PROF_MARK(1);
                    if (tid < 28) {
                        if (tid == 0) currentChi = iniChi = red[0];
                        else if (tid < 22) Hs[tid - 1] = red[tid];
                        else bs[tid - 22] = red[tid];
                    }
                } else {
                    ORBGPU_PROF_MARK(3);
                    if (haveSys && tid < 28) sysN[tid] = red[tid];
                    if (specPass) {
                        // candidate 0 rejected: the speculative candidates' robust chi2 in one pass,
                        // then their trials in order while they are rejected
                        pose_pass<kPoseSpec>([&](const PoseEdgeD& e, int i, double* v) {
#pragma unroll
                            for (int L = 1; L <= kPoseSpec; L++) {
                                double e3[3];
                                pose_err(e, Tc[L], P, e3);
                                v[L - 1] = pose_rho0(e, pose_chi2(e, e3), (fl[i] & 2) != 0);
                            }
                        }, na, aE, E, dM, dS, cs, red, myE, myIdx);
                        if (tid == 0)
                            for (int j = 1; j <= kPoseSpec && again && okc[j]; j++) trial(j, red[j - 1]);
                        __syncthreads();
                    }
                    ORBGPU_PROF_MARK(4);
                    if (again) continue;   // the next trial of this iteration
                    __syncthreads();
                    if (term || ++kit == 10) break;
                    if (!haveSys) {   // the next iteration starts with a system pass at T
                        sysPhase = true;
                        continue;
                    }
                    if (tid < 28) {   // the system at this estimate came with its accepted trial
                        if (tid == 0) currentChi = iniChi = sysN[0];
                        else if (tid < 22) Hs[tid - 1] = sysN[tid];
                        else bs[tid - 22] = sysN[tid];
                    }
                }
                // iteration start (Hs, bs, currentChi = iniChi are the system at T)
                __syncthreads();
                if (tid == 0) {
                    if (kit == 0) {   // computeLambdaInit over the pose diagonal
                        double mx = 0.;
                        for (int j = 0; j < 6; j++) mx = fmax(fabs(Hs[DIAG21[j]]), mx);
                        lambda = 1e-5 * mx;
                        ni = 2;
                        nBadLM = 0;
                    }
                    qmax = 0;
                    haveSys = 0;
                    Tbase = T;   // the estimate every trial of this iteration starts from
                }
                sysPhase = false;
                __syncthreads();
            }
        }
        // classification (Optimizer.cc:376-426): outliers get their error recomputed
        if (tid == 0) nBad = 0;
        __syncthreads();
        int mybad = 0;
        for (int i = tid; i < ne; i += blockDim.x) {
            const PoseEdgeD e = pose_edge_load(E, i, dM, dS);
            // active edges keep the error of the last pass (recomputed: the same operations on
            // the same pose), outliers get computeError() at the final estimate
            double e3[3];
            pose_err(e, outl[i] ? T : Terr, P, e3);
            const float chi2 = (float)pose_chi2(e, e3);
            uint8_t f = fl[i];
            if (chi2 > (e.stereo ? chi2Stereo : chi2Mono)) {
                outl[i] = 1;
                f |= 1;
                mybad++;
            } else {
                outl[i] = 0;
                f &= 2;
            }
            if (it == 2) f &= 1;   // setRobustKernel(0)
            fl[i] = f;
        }
        if (mybad) atomicAdd(&nBad, mybad);
        __syncthreads();
        if (ne < 10) break;   // optimizer.edges().size() < 10
    }
    if (tid == 0) {
        P.T = T;
        P.nbad = nBad;
        if (P.ninl) *P.ninl = ne - nBad;
    }
    if (P.Tcw_out) {   // pFrame->SetPose(Converter::toCvMat(SE3quat_recov)); mvbOutlier
        if (tid == 0) {
            se3_to_Tcw(T, P.Tcw_out);
            __threadfence_system();   // see the ne < 3 exit above: host-visible before the workgroup ends
        }
        for (int i = tid; i < ne; i += blockDim.x) P.outlier[E[i].meta & 0x7fffffff] = outl[i];
    }
}

// ---------------------------------------------------------------- test-only entries' kernels
// orbgpu_unit_se3: one item per thread through ba_math.hpp's inline functions.  SE3 rows are 7
// doubles (q xyzw, t).
__device__ __forceinline__ Se3 se3_row_load(const double* r) {
    Se3 s;
    for (int k = 0; k < 4; k++) s.q[k] = r[k];
    for (int k = 0; k < 3; k++) s.t[k] = r[4 + k];
    s.pad = 0;
    return s;
}
__device__ __forceinline__ void se3_row_store(const Se3& s, double* r) {
    for (int k = 0; k < 4; k++) r[k] = s.q[k];
    for (int k = 0; k < 3; k++) r[4 + k] = s.t[k];
}
__global__ void __launch_bounds__(256) k_unit_se3(int op, int n, const void* a, const void* b, void* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* A = (const double*)a;
    const double* B = (const double*)b;
    double* O = (double*)out;
    if (op == 0) {
        Se3 o;
        se3_exp(A + 6 * (size_t)i, o);
        se3_row_store(o, O + 7 * (size_t)i);
    } else if (op == 1) {
        Se3 o;
        se3_mul(se3_row_load(A + 7 * (size_t)i), se3_row_load(B + 7 * (size_t)i), o);
        se3_row_store(o, O + 7 * (size_t)i);
    } else if (op == 2) {
        double X[3], p[3];
        for (int k = 0; k < 3; k++) X[k] = B[3 * (size_t)i + k];
        se3_map(se3_row_load(A + 7 * (size_t)i), X, p);
        for (int k = 0; k < 3; k++) O[3 * (size_t)i + k] = p[k];
    } else if (op == 3) {
        float T[16];
        for (int k = 0; k < 16; k++) T[k] = ((const float*)a)[16 * (size_t)i + k];
        Se3 o;
        se3_from_Tcw(T, o);
        se3_row_store(o, O + 7 * (size_t)i);
    } else {
        float T[16];
        se3_to_Tcw(se3_row_load(A + 7 * (size_t)i), T);
        for (int k = 0; k < 16; k++) ((float*)out)[16 * (size_t)i + k] = T[k];
    }
}

// orbgpu_unit_pose_stage: one linearisation at T0 and one LM trial at a given lambda, one
// workgroup, through k_pose_opt's own device functions.  out (doubles; integers and floats are
// stored exactly): head = sums 28 | x 6 | T0 7 | T_trial 7 | the trial's sum of rho | scale |
// nA | ok | Tcw_trial 16, then one row per edge = err 3 | chi2e | rho | J 18 | terms 28 |
// chi2e_trial | rho_trial | the classification's float chi2 at T_trial | keypoint.  Rows of
// inactive edges keep what the host put there, except the last two columns.
constexpr int kStageHead = 68, kStageCols = 55;
template <int NT>
__global__ void __launch_bounds__(NT) k_pose_stage(const PoseProbDev* probs, const PoseEdgeDev* __restrict__ E,
                                                   const uint8_t* flags, double lam, double* out) {
    const PoseProbDev& P = probs[0];
    const int ne = P.ne, tid = threadIdx.x;
    __shared__ uint8_t fl[kPoseMaxEdges];
    __shared__ uint16_t aE[kPoseMaxEdges];
    __shared__ double cs[28][kPoseMaxEdges / 64];
    __shared__ double red[32], sums[28], scr[36], xs[6];
    __shared__ Se3 T0, Tt;
    __shared__ int nA, wsum[16];
    const double dM = (double)(float)sqrt(5.991), dS = (double)(float)sqrt(7.815);
    double* rows = out + kStageHead;
    for (int i = tid; i < ne; i += NT) {
        fl[i] = flags[i];
        rows[(size_t)i * kStageCols + 54] = (double)(E[i].meta & 0x7fffffff);
    }
    if (tid == 0) {
        T0 = P.T0;
        for (int j = 0; j < 6; j++) xs[j] = 0.0;   // k_pose_opt's xs at the start of a round
    }
    __syncthreads();
    pose_compact<NT>(fl, ne, aE, wsum, &nA);
    const int na = nA;
    const int myIdx = tid < na ? aE[tid] : 0;
    const PoseEdgeD myE = pose_edge_load(E, myIdx, dM, dS);
    for (int phase = 0; phase < 2; phase++) {   // 0: the system at T0; 1: the trial's pass at T_trial
        const Se3& X = phase ? Tt : T0;
        pose_pass<28>([&](const PoseEdgeD& e, int i, double* v) {
            double J[18], e3[3];
            pose_sys_terms_je(e, (fl[i] & 2) != 0, X, P, v, J, e3);
            double* r = rows + (size_t)i * kStageCols;
            const double c = pose_chi2(e, e3);
            if (phase == 0) {
                for (int k = 0; k < 3; k++) r[k] = e3[k];
                r[3] = c;
                r[4] = v[0];
                for (int k = 0; k < 18; k++) r[5 + k] = J[k];
                for (int k = 0; k < 28; k++) r[23 + k] = v[k];
            } else {
                r[51] = c;
                r[52] = v[0];
            }
        }, na, aE, E, dM, dS, cs, red, myE, myIdx);
        if (phase == 1) {
            if (tid == 0) out[48] = red[0];
            break;
        }
        if (tid < 28) {
            sums[tid] = red[tid];
            out[tid] = red[tid];
        }
        __syncthreads();
        if (tid < 64) {   // k_pose_opt's candidate 0: solve, step from xs when the solve fails
            double xn[6], xl[6];
            const bool ok = pose_solve_l(sums + 1, sums + 22, lam, xn, scr);
#pragma unroll
            for (int j = 0; j < 6; j++) xl[j] = ok ? xn[j] : xs[j];
            Se3 d, r;
            se3_exp(xl, d);
            se3_mul(d, T0, r);
            if (tid == 0) {
                Tt = r;
                double sv[6];
                for (int q = 0; q < 6; q++) {
                    out[28 + q] = xl[q];
                    sv[q] = xl[q] * (lam * xl[q] + sums[22 + q]);
                }
                out[49] = tree64_local([&](int q) { return sv[q]; }, 6);
                out[50] = (double)na;
                out[51] = ok ? 1.0 : 0.0;
            }
        }
        __syncthreads();
    }
    // the classification's chi2 (Optimizer.cc:376-426) at the pose of the last pass
    for (int i = tid; i < ne; i += NT) {
        const PoseEdgeD e = pose_edge_load(E, i, dM, dS);
        double e3[3];
        pose_err(e, Tt, P, e3);
        rows[(size_t)i * kStageCols + 53] = (double)(float)pose_chi2(e, e3);
    }
    if (tid == 0) {
        se3_row_store(T0, out + 34);
        se3_row_store(Tt, out + 41);
        float o[16];
        se3_to_Tcw(Tt, o);
        for (int k = 0; k < 16; k++) out[52 + k] = (double)o[k];
    }
}

// Device mode edge creation (Optimizer.cc:268-347): rows with a map point, keypoint order,
// compacted by a block scan; the initial pose from the frame's Tcw.  One workgroup per frame.
// 4 waves: the pack fits in the slot of one retiring extraction workgroup
constexpr int kPackThreads = 256;
__global__ void __launch_bounds__(kPackThreads) k_pose_pack(PoseProbDev* probs, PoseEdgeDev* Eall) {
    ORBGPU_LATENCY_WAVE();
    PoseProbDev& P = probs[blockIdx.x];
    const int N = P.N, tid = threadIdx.x;
    PoseEdgeDev* E = Eall + P.e0;
    __shared__ int wsum[kPackThreads / 64], base;
    if (tid == 0) {
        base = 0;
        se3_from_Tcw(P.Tcw, P.T0);
    }
    __syncthreads();
    for (int c0 = 0; c0 < N; c0 += kPackThreads) {
        const int i = c0 + tid;
        const int f = i < N ? (P.mpidx ? (P.mpidx[i] >= 0 ? 1 : 0) : (P.has_mp[i] ? 1 : 0)) : 0;
        int incl = f;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if ((tid & 63) >= o) incl += t;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        int off = base;
        for (int w = 0; w < (tid >> 6); w++) off += wsum[w];
        if (f) {
            const int k = off + incl - 1;
            if (k < kPoseMaxEdges) {
                PoseEdgeDev e;
                if (P.mpidx) {
                    // Optimizer.cc:268-347: pMP->GetWorldPos(), kpUn.pt, mvuRight, mvInvLevelSigma2[kpUn.octave]
                    const size_t m = (size_t)P.mpidx[i];
                    for (int j = 0; j < 3; j++) e.Xw[j] = P.mp_pos[3 * m + j];
                    e.obs[0] = P.keys[7 * (size_t)i];
                    e.obs[1] = P.keys[7 * (size_t)i + 1];
                    e.obs[2] = P.uR[i];
                    const int oct = min(max(__float_as_int(P.keys[7 * (size_t)i + 5]), 0), P.nlev - 1);
                    e.info = P.isig_tab[oct];
                } else {
                    for (int j = 0; j < 3; j++) {
                        e.Xw[j] = P.Xw[3 * i + j];
                        e.obs[j] = P.obs[3 * i + j];
                    }
                    e.info = P.inv_sigma2[i];
                }
                e.meta = i | (!(e.obs[2] < 0) ? (int)0x80000000u : 0);
                E[k] = e;
            }
        }
        __syncthreads();
        if (tid == kPackThreads - 1) base = off + incl;
        __syncthreads();
    }
    if (tid == 0) P.ne = base > kPoseMaxEdges ? -1 : base;
}

// ---------------------------------------------------------------- PoseEngine
int PoseEngine::run_device(int count, const pose_problem* P, float* const* Tcw_out, uint8_t* const* outlier,
                           int* ninliers) {
    std::vector<int> Ns(count);
    for (int f = 0; f < count; f++) Ns[f] = P[f].N;
    return launch_device(count, Ns.data(), [&](int f, PoseProbDev& pp) {
        const pose_problem& Q = P[f];
        pp.fx = Q.fx; pp.fy = Q.fy; pp.cx = Q.cx; pp.cy = Q.cy; pp.bf = Q.bf;
        pp.Tcw = Q.Tcw; pp.has_mp = Q.has_mp; pp.Xw = Q.Xw; pp.obs = Q.obs; pp.inv_sigma2 = Q.inv_sigma2;
    }, Tcw_out, outlier, ninliers);
}

int PoseEngine::run_frames_device(int count, const pose_frame* F, float* const* Tcw_out, uint8_t* const* outlier,
                                  int* ninliers, hipStream_t s, DeferredChain* chain) {
    std::vector<int> Ns(count);
    for (int f = 0; f < count; f++) Ns[f] = F[f].N;
    return launch_device(count, Ns.data(), [&](int f, PoseProbDev& pp) {
        const pose_frame& Q = F[f];
        pp.fx = Q.fx; pp.fy = Q.fy; pp.cx = Q.cx; pp.cy = Q.cy; pp.bf = Q.bf;
        pp.Tcw = Q.Tcw;
        pp.mpidx = Q.mp; pp.mp_pos = Q.mp_pos; pp.keys = (const float*)Q.keysUn; pp.uR = Q.uRight;
        pp.isig_tab = Q.invLevelSigma2; pp.nlev = Q.nlevels;
    }, Tcw_out, outlier, ninliers, s, chain);
}

// Device-mode launch.  Default: own stream, results synchronised before return.  With a
// DeferredChain: enqueued on `s` behind the caller's previous work, the problem table staged
// through the chain's pinned blocks and the inlier counts landing in `ninliers` at
// chain.finish() (-1 for a frame over kPoseMaxEdges).
int PoseEngine::launch_device(int count, const int* Ns, const std::function<void(int, PoseProbDev&)>& fill,
                              float* const* Tcw_out, uint8_t* const* outlier, int* ninliers, hipStream_t s,
                              DeferredChain* chain) {
    hipStream_t st = s ? s : stream_;
    size_t nmax = 0;
    for (int f = 0; f < count; f++) nmax += (size_t)std::min(Ns[f], kPoseMaxEdges + 1);
    const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bProb = al(sizeof(PoseProbDev) * count), bEdge = al(sizeof(PoseEdgeDev) * std::max<size_t>(nmax, 1));
    const size_t bOut = al(std::max<size_t>(nmax, 1)), bNin = al(sizeof(int) * count);
    const size_t need = bProb + bEdge + bOut + bNin;
    if (need > cap_) {
        if (lastUseSet_) ORB_HIP_CHECK(hipEventSynchronize(lastUse_));   // queued kernels may still read it
        if (dArena_) (void)hipFree(dArena_);
        if (hArena_) (void)hipHostFree(hArena_);
        dArena_ = hArena_ = nullptr;
        cap_ = 0;
        ORB_HIP_CHECK(hipMalloc(&dArena_, need));
        ORB_HIP_CHECK(hipHostMalloc(&hArena_, need));
        cap_ = need;
    }
    char* d = (char*)dArena_;
    // inlier counts: the arena, or in a chain its count blocks (copied when the chain closes)
    int* dNin = chain ? (int*)chain->dev_counts(sizeof(int) * count) : (int*)(d + bProb + bEdge + bOut);
    if (!dNin) return -2;
    std::vector<PoseProbDev> tmp;
    PoseProbDev* hp = (PoseProbDev*)hArena_;
    if (chain) {   // hArena_ may still be the source of an earlier queued copy: stage instead
        tmp.resize(count);
        hp = tmp.data();
    }
    size_t e0 = 0;
    for (int f = 0; f < count; f++) {
        PoseProbDev& pp = hp[f];
        memset(&pp, 0, sizeof(pp));
        pp.N = Ns[f];
        pp.e0 = (int)e0;
        e0 += (size_t)std::min(Ns[f], kPoseMaxEdges + 1);
        fill(f, pp);
        pp.Tcw_out = Tcw_out[f];
        pp.outlier = outlier[f];
        pp.ninl = dNin + f;
    }
    PoseProbDev* dp = (PoseProbDev*)d;
    PoseEdgeDev* dE = (PoseEdgeDev*)(d + bProb);
    const void* src = chain ? chain->stage(hp, sizeof(PoseProbDev) * count) : (const void*)hp;
    if (!src) return -2;
    // the arena's previous user may be queued on another stream (a deferred chain of another
    // matcher, or this engine's own stream): overwrite the problem table only after it is done
    if (lastUseSet_) ORB_HIP_CHECK(hipStreamWaitEvent(st, lastUse_, 0));
    ORB_HIP_CHECK(hipMemcpyAsync(d, src, sizeof(PoseProbDev) * count, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pose_pack, dim3(count), dim3(kPackThreads), 0, st, dp, dE);
    if (timing_) ORB_HIP_CHECK(hipEventRecord(tA_, st));
    if (count <= pose_wide_max())
        hipLaunchKernelGGL(k_pose_opt<kPoseThreadsWide>, dim3(count), dim3(kPoseThreadsWide),
                           pose_lds_pad((const void*)k_pose_opt<kPoseThreadsWide>), st, dp, (const PoseEdgeDev*)dE,
                           nullptr, (uint8_t*)(d + bProb + bEdge));
    else
        hipLaunchKernelGGL(k_pose_opt<kPoseThreads>, dim3(count), dim3(kPoseThreads),
                           pose_lds_pad((const void*)k_pose_opt<kPoseThreads>), st, dp, (const PoseEdgeDev*)dE, nullptr,
                           (uint8_t*)(d + bProb + bEdge));
    ORB_HIP_CHECK(hipGetLastError());
    if (timing_) {
        ORB_HIP_CHECK(hipEventRecord(tB_, st));
        timed_ = true;
    }
    if (chain) {
        chain->land_dev(ninliers, dNin, sizeof(int) * count);
        ORB_HIP_CHECK(hipEventRecord(lastUse_, st));
        lastUseSet_ = true;
        return 0;
    }
    ORB_HIP_CHECK(hipMemcpyAsync(hp, d, bProb, hipMemcpyDeviceToHost, st));
    ORB_HIP_CHECK(hipEventRecord(lastUse_, st));
    lastUseSet_ = true;
    ORB_HIP_CHECK(stream_wait(st));
    int rc = 0;
    for (int f = 0; f < count; f++) {
        const PoseProbDev& pp = hp[f];
        if (pp.ne < 0) rc = -3;
        ninliers[f] = pp.ne < 0 || pp.nbad < 0 ? 0 : pp.ne - pp.nbad;
    }
    return rc;
}

int PoseEngine::last_timing(float* ms) {
    if (!timed_) return -1;
    ORB_HIP_CHECK(hipEventSynchronize(tB_));
    ORB_HIP_CHECK(hipEventElapsedTime(ms, tA_, tB_));
    return 0;
}

PoseEngine::~PoseEngine() {
    if (lastUseSet_) (void)hipEventSynchronize(lastUse_);
    if (lastUse_) (void)hipEventDestroy(lastUse_);
    if (tA_) (void)hipEventDestroy(tA_);
    if (tB_) (void)hipEventDestroy(tB_);
    if (dArena_) (void)hipFree(dArena_);
    if (hArena_) (void)hipHostFree(hArena_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

int PoseEngine::init() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -4;
    ORB_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    ORB_HIP_CHECK(hipEventCreateWithFlags(&lastUse_, hipEventDisableTiming));
    ORB_HIP_CHECK(hipEventCreate(&tA_));
    ORB_HIP_CHECK(hipEventCreate(&tB_));
    return 0;
}

// Edge creation on the host (Optimizer.cc:268-347): rows with a map point in keypoint order
static int pose_edges_host(const pose_problem& Q, PoseEdgeDev* he) {
    int k = 0;
    for (int i = 0; i < Q.N; i++) {
        if (!Q.has_mp[i]) continue;
        PoseEdgeDev& e = he[k++];
        for (int j = 0; j < 3; j++) {
            e.Xw[j] = Q.Xw[3 * i + j];
            e.obs[j] = Q.obs[3 * i + j];
        }
        e.info = Q.inv_sigma2[i];
        e.meta = i | (!(Q.obs[3 * i + 2] < 0) ? (int)0x80000000u : 0);
    }
    return k;
}

// Edge creation (Optimizer.cc:268-347): rows with a map point in keypoint order.
int PoseEngine::run(int count, const pose_problem* P, float* Tcw_out, uint8_t* const* outlier, int* ninliers) {
    size_t ne = 0;
    std::vector<int> nE(count);
    for (int f = 0; f < count; f++) {
        int c = 0;
        for (int i = 0; i < P[f].N; i++) c += P[f].has_mp[i] ? 1 : 0;
        if (c > kPoseMaxEdges) return -3;
        nE[f] = c;
        ne += c;
    }
    const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bProb = al(sizeof(PoseProbDev) * count), bEdge = al(sizeof(PoseEdgeDev) * std::max<size_t>(ne, 1));
    const size_t bErr = al(sizeof(double) * 3 * std::max<size_t>(ne, 1)), bOut = al(std::max<size_t>(ne, 1));
    const size_t need = bProb + bEdge + bErr + bOut;
    if (lastUseSet_) ORB_HIP_CHECK(hipEventSynchronize(lastUse_));   // hArena_ / dArena_ free again
    if (need > cap_) {
        if (dArena_) (void)hipFree(dArena_);
        if (hArena_) (void)hipHostFree(hArena_);
        dArena_ = hArena_ = nullptr;
        cap_ = 0;
        ORB_HIP_CHECK(hipMalloc(&dArena_, need));
        ORB_HIP_CHECK(hipHostMalloc(&hArena_, need));
        cap_ = need;
    }
    char* h = (char*)hArena_;
    char* d = (char*)dArena_;
    PoseProbDev* hp = (PoseProbDev*)h;
    PoseEdgeDev* he = (PoseEdgeDev*)(h + bProb);
    uint8_t* hOut = (uint8_t*)(h + bProb + bEdge + bErr);
    int e0 = 0;
    for (int f = 0; f < count; f++) {
        const pose_problem& Q = P[f];
        PoseProbDev& pp = hp[f];
        memset(&pp, 0, sizeof(pp));
        pp.ne = nE[f];
        pp.e0 = e0;
        host_se3_from_Tcw(Q.Tcw, pp.T0);
        pp.fx = Q.fx; pp.fy = Q.fy; pp.cx = Q.cx; pp.cy = Q.cy; pp.bf = Q.bf;
        e0 += pose_edges_host(Q, he + e0);
    }
    PoseProbDev* dp = (PoseProbDev*)d;
    ORB_HIP_CHECK(hipMemcpyAsync(d, h, bProb + sizeof(PoseEdgeDev) * ne, hipMemcpyHostToDevice, stream_));
    if (count > 0)
    {
        if (count <= pose_wide_max())
            hipLaunchKernelGGL(k_pose_opt<kPoseThreadsWide>, dim3(count), dim3(kPoseThreadsWide), 0, stream_, dp, (const PoseEdgeDev*)(d + bProb),
                               (double*)(d + bProb + bEdge), (uint8_t*)(d + bProb + bEdge + bErr));
        else
            hipLaunchKernelGGL(k_pose_opt<kPoseThreads>, dim3(count), dim3(kPoseThreads), 0, stream_, dp, (const PoseEdgeDev*)(d + bProb),
                               (double*)(d + bProb + bEdge), (uint8_t*)(d + bProb + bEdge + bErr));
    }
    ORB_HIP_CHECK(hipGetLastError());
    ORB_HIP_CHECK(hipMemcpyAsync(h, d, bProb, hipMemcpyDeviceToHost, stream_));
    if (ne) ORB_HIP_CHECK(hipMemcpyAsync(hOut, d + bProb + bEdge + bErr, ne, hipMemcpyDeviceToHost, stream_));
    ORB_HIP_CHECK(hipEventRecord(lastUse_, stream_));
    lastUseSet_ = true;
    ORB_HIP_CHECK(hipStreamSynchronize(stream_));
    for (int f = 0; f < count; f++) {
        const pose_problem& Q = P[f];
        const PoseProbDev& pp = hp[f];
        const uint8_t* o = hOut + pp.e0;
        for (int i = 0, k = 0; i < Q.N; i++)
            if (Q.has_mp[i]) {
                outlier[f][i] = pp.nbad < 0 ? 0 : o[k];
                k++;
            }
        if (pp.nbad < 0) {   // nInitialCorrespondences < 3: return 0, pose untouched
            memcpy(Tcw_out + 16 * (size_t)f, Q.Tcw, sizeof(float) * 16);
            ninliers[f] = 0;
        } else {
            host_se3_to_Tcw(pp.T, Tcw_out + 16 * (size_t)f);
            ninliers[f] = pp.ne - pp.nbad;
        }
    }
    return 0;
}

// ---------------------------------------------------------------- test-only entries
int pose_unit_se3(int op, int n, const void* a, const void* b, void* out) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return -4;
    if (n == 0) return 0;
    const size_t bA = (op == 0 ? 6 * sizeof(double) : op == 3 ? 16 * sizeof(float) : 7 * sizeof(double)) * (size_t)n;
    const size_t bB = (op == 1 ? 7 : op == 2 ? 3 : 0) * sizeof(double) * (size_t)n;
    const size_t bO = (op == 2 ? 3 * sizeof(double) : op == 4 ? 16 * sizeof(float) : 7 * sizeof(double)) * (size_t)n;
    const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char* dm = nullptr;
    ORB_HIP_CHECK(hipMalloc((void**)&dm, al(bA) + al(bB) + bO));
    char *dA = dm, *dB = dA + al(bA), *dO = dB + al(bB);
    int rc = 0;
    if (hipMemcpy(dA, a, bA, hipMemcpyHostToDevice) != hipSuccess) rc = -2;
    if (!rc && bB && hipMemcpy(dB, b, bB, hipMemcpyHostToDevice) != hipSuccess) rc = -2;
    if (!rc) {
        hipLaunchKernelGGL(k_unit_se3, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, (const void*)dA, (const void*)dB,
                           (void*)dO);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dO, bO, hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
    }
    (void)hipFree(dm);
    return rc;
}

int pose_stage_run(const pose_problem* Q, const uint8_t* flags, double lambda, int threads, pose_stage* out) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return -4;
    int ne = 0;
    for (int i = 0; i < Q->N; i++) ne += Q->has_mp[i] ? 1 : 0;
    if (ne > kPoseMaxEdges) return -3;
    out->ne = ne;
    out->nA = out->ok = 0;
    if (ne == 0) return 0;
    PoseProbDev pp;
    memset(&pp, 0, sizeof(pp));
    pp.ne = ne;
    host_se3_from_Tcw(Q->Tcw, pp.T0);
    pp.fx = Q->fx; pp.fy = Q->fy; pp.cx = Q->cx; pp.cy = Q->cy; pp.bf = Q->bf;
    std::vector<PoseEdgeDev> he(ne);
    pose_edges_host(*Q, he.data());
    const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t bP = al(sizeof(pp)), bE = al(sizeof(PoseEdgeDev) * ne), bF = al((size_t)ne);
    const size_t nOut = kStageHead + (size_t)kStageCols * ne;
    char* dm = nullptr;
    ORB_HIP_CHECK(hipMalloc((void**)&dm, bP + bE + bF + sizeof(double) * nOut));
    double* dO = (double*)(dm + bP + bE + bF);
    std::vector<double> ho(nOut);
    int rc = 0;
    if (hipMemcpy(dm, &pp, sizeof(pp), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dm + bP, he.data(), sizeof(PoseEdgeDev) * ne, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dm + bP + bE, flags, ne, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dO, 0xff, sizeof(double) * nOut) != hipSuccess)   // NaN wherever the kernel writes nothing
        rc = -2;
    if (!rc) {
        if (threads == kPoseThreadsWide)
            hipLaunchKernelGGL(k_pose_stage<kPoseThreadsWide>, dim3(1), dim3(kPoseThreadsWide), 0, 0,
                               (const PoseProbDev*)dm, (const PoseEdgeDev*)(dm + bP), (const uint8_t*)(dm + bP + bE),
                               lambda, dO);
        else
            hipLaunchKernelGGL(k_pose_stage<kPoseThreads>, dim3(1), dim3(kPoseThreads), 0, 0, (const PoseProbDev*)dm,
                               (const PoseEdgeDev*)(dm + bP), (const uint8_t*)(dm + bP + bE), lambda, dO);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpy(ho.data(), dO, sizeof(double) * nOut, hipMemcpyDeviceToHost) != hipSuccess)
            rc = -2;
    }
    (void)hipFree(dm);
    if (rc) return rc;
    const double* h = ho.data();
    out->nA = (int)h[50];
    out->ok = (int)h[51];
    out->chi2_trial = h[48];
    out->scale = h[49];
    const auto put = [&](double* dst, int col, int w) {
        if (!dst) return;
        for (int i = 0; i < ne; i++)
            for (int k = 0; k < w; k++) dst[(size_t)i * w + k] = h[kStageHead + (size_t)i * kStageCols + col + k];
    };
    put(out->err, 0, 3);
    put(out->chi2e, 3, 1);
    put(out->rho, 4, 1);
    put(out->J, 5, 18);
    put(out->terms, 23, 28);
    put(out->chi2e_trial, 51, 1);
    put(out->rho_trial, 52, 1);
    for (int i = 0; i < ne; i++) {
        const double* r = h + kStageHead + (size_t)i * kStageCols;
        if (out->chi2_class) out->chi2_class[i] = (float)r[53];
        if (out->keypoint) out->keypoint[i] = (int32_t)r[54];
    }
    const auto head = [&](double* dst, int o, int w) {
        if (dst) memcpy(dst, h + o, sizeof(double) * w);
    };
    head(out->sums, 0, 28);
    head(out->x, 28, 6);
    head(out->T0, 34, 7);
    head(out->T_trial, 41, 7);
    if (out->Tcw_trial)
        for (int k = 0; k < 16; k++) out->Tcw_trial[k] = (float)h[52 + k];
    return 0;
}

}  // namespace orbgpu
