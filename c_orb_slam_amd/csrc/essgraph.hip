// essgraph.hip -- gfx950 Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044):
// the Sim3 pose graph over the essential graph that LoopClosing::CorrectLoop (LoopClosing.cc:567)
// runs between the loop fusion and the global BA.
//
// One VertexSim3Expmap per keyframe, EdgeSim3 (information I7, no robust kernel) with g2o's
// numeric central-difference Jacobians (delta 1e-9), BlockSolver_7_3 without marginalised
// vertices: H (7x7 blocks) is solved directly.  Per LM iteration:
//   - k_ess_lin: a work item is (edge, evaluation): 32 lanes per edge, lane 28 the error, lanes
//     2d + 14 side and + 1 the +-delta errors of column d of vertex `side` (adjacent lanes, the
//     difference is one cross-lane move); writes e, chi2_e, J_i, J_j (the errors-only pass of a
//     trial writes chi2_e alone, so e stays the linearisation point's for every retry);
//   - per trial: k_ess_assemble gathers each 7x7 block of H (and b) from the host-built edge
//     lists in edge order (no float atomics: sums are identical run to run), adds lambda and
//     writes the dense matrix or the tiles of the block-sparse solver (groups of 7 rows);
//     the dense single-workgroup LDL^T (n <= kDenseMaxN) or SparseLdlt solves; k_ess_update
//     backs the estimates up and applies exp(x) * estimate; an errors-only k_ess_lin and the
//     canonical tree sums give the trial's chi2 and computeScale;
//   - the host takes the accept / reject decision from the four scalars (lm_control.hpp, the one
//     BaEngine::lm_solve uses).
// Finish kernels: CorrectedSiw^-1, Tcw = [R | t/s] as float, and the map-point correction.
// Test-only entries (orbgpu_unit_essgraph_stage, orbgpu_unit_sim3): one linearisation and one
// trial through the same launches with every intermediate buffer copied out, and the Sim3
// functions one item per thread.
#include "essgraph.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "ba_math.hpp"
#include "detmath.hpp"
#include "ldlt.hpp"
#include "lm_control.hpp"
#include "orb_common.hpp"
#include "sim3_math.hpp"

namespace orbgpu {

constexpr int kEssLanes = 32;                  // lanes per edge in k_ess_lin
constexpr int kEssEdgesPerBlock = 256 / kEssLanes;
constexpr int kEssJ = 98;                      // doubles of (J_i, J_j) per edge: [side][row k][column d]
constexpr int kEssSumMaxChunks = 7168;         // k_ess_sum's LDS scratch (57 KiB): n <= 458752

// S(r, c), r <= c in system order, groups of 7 rows (SysAddr with the pose graph's group size)
struct EssAddr {
    double* dense;
    int nn;
    const int* slot_of;
    double* tiles;
    int nt;
    const int* prow;
    __device__ __forceinline__ double* at(int r, int c) const {
        if (dense) return dense + (size_t)r * nn + c;
        int a = prow[r / 7] + r % 7, b = prow[c / 7] + c % 7;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int s = slot_of[(size_t)(a >> 6) * nt + (b >> 6)];
        return tiles + (size_t)s * (kTile * kTile) + (a & 63) * kTile + (b & 63);
    }
};

struct EssDev {
    int nKF, nE, fix;
    const Sim3d* est;
    const Sim3d* meas;
    const int32_t *ei, *ej;
    const uint8_t* fixed;
    double *err, *chi2e, *J;
};

// measurement Sji = Sjw * Swi: both from vScw on a LoopConnections edge, else from the
// non-corrected table (Optimizer.cc:866-871, 905-960)
__global__ void __launch_bounds__(256) k_ess_meas(int nE, const int32_t* ei, const int32_t* ej, const uint8_t* loop,
                                                  const Sim3d* Scw, const Sim3d* Snc, Sim3d* meas) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nE) return;
    const Sim3d* tab = loop[e] ? Scw : Snc;
    const Sim3d Siw = tab[ei[e]], Sjw = tab[ej[e]];
    Sim3d Swi, m;
    sim3_inverse(Siw, Swi);
    sim3_mul(Sjw, Swi, m);
    meas[e] = m;
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:96-103): log(C * v1 * v2^-1)
__device__ __forceinline__ void ess_error(const Sim3d& M, const Sim3d& Si, const Sim3d& Sj, double* e7) {
    Sim3d Sji, A, E;
    sim3_inverse(Sj, Sji);
    sim3_mul(M, Si, A);
    sim3_mul(A, Sji, E);
    sim3_log(E, e7);
}

// full = 1: computeActiveErrors + BaseBinaryEdge::linearizeOplus (numeric); 0: errors only
__global__ void __launch_bounds__(256) k_ess_lin(EssDev P, int full) {
    const int e = blockIdx.x * kEssEdgesPerBlock + (threadIdx.x / kEssLanes);
    const int l = threadIdx.x % kEssLanes;
    const bool edgeOk = e < P.nE;
    const int ec = edgeOk ? e : P.nE - 1;
    const int vi = P.ei[ec], vj = P.ej[ec];
    const int side = l >= 14 ? 1 : 0, d = (l - 14 * side) >> 1;
    const bool pert = full && l < 28 && !P.fixed[side ? vj : vi];
    const bool base = l == 28;
    const bool active = edgeOk && (pert || base);
    double ev[7] = {0, 0, 0, 0, 0, 0, 0};
    if (active) {
        Sim3d Si = P.est[vi], Sj = P.est[vj];
        if (pert) {   // push / oplus(+-delta e_d) / pop on one vertex
            double add[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 7; j++)
                if (j == d) add[j] = (l & 1) ? -1e-9 : 1e-9;
            if (P.fix) add[6] = 0;   // oplusImpl: _fix_scale
            Sim3d U;
            sim3_exp(add, U);
            if (side) sim3_mul(U, Sj, Sj);
            else sim3_mul(U, Si, Si);
        }
        ess_error(P.meas[ec], Si, Sj, ev);
    }
    if (full) {
        const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const double other = __shfl_xor(ev[k], 1, 64);   // the -delta error of the pair
            if (active && pert && !(l & 1)) P.J[(size_t)e * kEssJ + side * 49 + k * 7 + d] = scalar * (ev[k] - other);
        }
    }
    if (edgeOk && base) {
        double c = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            // a trial's errors-only pass leaves the linearisation point's e alone: every retry of
            // the iteration assembles b = -J^T e from it
            if (full) P.err[(size_t)e * 7 + k] = ev[k];
            c += ev[k] * ev[k];
        }
        P.chi2e[e] = c;
    }
}

// One workgroup per 7x7 block of H, upper triangle in system order: diagonal blocks (a == b) sum
// J^T J over the vertex's edges, add lambda and form b = -J^T e; off-diagonal blocks (a < b) sum
// J_a^T J_b over the pair's edges.  ent = 2 * edge + side of vertex a (0: vertex(0) = i).
__global__ void __launch_bounds__(64) k_ess_assemble(const int* blkStart, const int* blkA, const int* blkB,
                                                     const int* ent, const double* J, const double* err,
                                                     double lambda, EssAddr sa, double* bvec) {
    const int blk = blockIdx.x, t = threadIdx.x;
    const int a = blkA[blk], b = blkB[blk];
    const bool diag = a == b;
    const int q0 = blkStart[blk], q1 = blkStart[blk + 1];
    if (t < 49) {
        const int r = t / 7, c = t % 7;
        double acc = 0;
        for (int q = q0; q < q1; q++) {
            const int en = ent[q], s = en & 1;
            const double* Ja = J + (size_t)(en >> 1) * kEssJ + s * 49;
            const double* Jb = diag ? Ja : J + (size_t)(en >> 1) * kEssJ + (1 - s) * 49;
            double h = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) h += Ja[k * 7 + r] * Jb[k * 7 + c];
            acc += h;
        }
        if (diag && r == c) acc += lambda;
        if (!diag || r <= c) *sa.at(7 * a + r, 7 * b + c) = acc;
    } else if (t < 56 && diag) {
        const int r = t - 49;
        double acc = 0;
        for (int q = q0; q < q1; q++) {
            const int en = ent[q];
            const double* Ja = J + (size_t)(en >> 1) * kEssJ + (en & 1) * 49;
            const double* ee = err + (size_t)(en >> 1) * 7;
            double g = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) g += Ja[k * 7 + r] * ee[k];
            acc -= g;
        }
        bvec[7 * a + r] = acc;
    }
}

// push + update: VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-68), the scale entry
// zeroed in the solver's x itself so that computeScale sees the zero
__global__ void __launch_bounds__(256) k_ess_update(int nKF, int fix, const int* sysIdx, Sim3d* est, Sim3d* bak,
                                                    double* x) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nKF) return;
    const Sim3d T = est[v];
    bak[v] = T;
    const int s = sysIdx[v];
    if (s < 0) return;
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = x[7 * s + k];
    if (fix) {
        u[6] = 0;
        x[7 * s + 6] = 0;
    }
    Sim3d U, M;
    sim3_exp(u, U);
    sim3_mul(U, T, M);
    est[v] = M;
}

// canonical (ora_csum) totals: mode 0 the chi2 of the edges, mode 1 computeScale's sum of
// x (lambda x + b).  The waves share the 64-term chunks of the first level; wave 0 sums the chunk
// totals the same way.  LDS: ceil(n / 64) chunk totals + the scratch of their sum.
constexpr int kEssSumThreads = 1024;
__global__ void __launch_bounds__(kEssSumThreads) k_ess_sum(int mode, int n, const double* a, const double* b,
                                                           double lambda, double* out) {
    extern __shared__ double sc[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int m = (n + 63) >> 6;
    const auto f = [&](int i) { return mode == 0 ? a[i] : a[i] * (lambda * a[i] + b[i]); };
    for (int c = w; c < m; c += nw) {
        const int i = c * 64 + lane;
        double v = i < n ? f(i) : 0.0;
        v = n == 1 ? v : wave_tree(v);   // ora_csum keeps a single term untouched
        if (lane == 0) sc[c] = v;
    }
    __syncthreads();
    if (w == 0) {
        const double t = wave_csum([&](int i) { return sc[i]; }, m, sc + m);
        if (lane == 0) *out = t;
    }
}

// vCorrectedSwc and the SetPose argument [R | t / s] (Optimizer.cc:985-1003)
__global__ void __launch_bounds__(256) k_ess_finish(int nKF, const Sim3d* est, Sim3d* Swc, float* Tcw) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nKF) return;
    const Sim3d T = est[v];
    Sim3d I;
    sim3_inverse(T, I);
    Swc[v] = I;
    double R[9];
    quat_to_R(T.q, R);
    float* o = Tcw + 16 * (size_t)v;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[r * 4 + c] = (float)R[r * 3 + c];
        o[r * 4 + 3] = (float)(T.t[r] * (1. / T.s));
    }
    o[12] = o[13] = o[14] = 0.f;
    o[15] = 1.f;
}

// map points: P <- correctedSwr.map(Srw.map(P)) (Optimizer.cc:1006-1042)
__global__ void __launch_bounds__(256) k_ess_points(int nMP, const int32_t* ref, const Sim3d* Scw, const Sim3d* Swc,
                                                    float* pos) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nMP) return;
    const int r = ref[p];
    if (r < 0) return;
    const double X[3] = {(double)pos[3 * (size_t)p], (double)pos[3 * (size_t)p + 1], (double)pos[3 * (size_t)p + 2]};
    double c[3], w[3];
    sim3_map(Scw[r], X, c);
    sim3_map(Swc[r], c, w);
    for (int i = 0; i < 3; i++) pos[3 * (size_t)p + i] = (float)w[i];
}

// ---------------------------------------------------------------- unit entries' kernels
// orbgpu_unit_sim3: one item per thread through the inline functions above
__global__ void __launch_bounds__(256) k_unit_sim3(int op, int n, const double* a, const double* b, const double* c,
                                                   double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Sim3d* A = (const Sim3d*)a;
    const Sim3d* B = (const Sim3d*)b;
    if (op == 0) {
        Sim3d o;
        sim3_exp(a + 7 * (size_t)i, o);
        ((Sim3d*)out)[i] = o;
    } else if (op == 1) {
        sim3_log(A[i], out + 7 * (size_t)i);
    } else if (op == 2) {
        Sim3d o;
        sim3_mul(A[i], B[i], o);
        ((Sim3d*)out)[i] = o;
    } else if (op == 3) {
        Sim3d o;
        sim3_inverse(A[i], o);
        ((Sim3d*)out)[i] = o;
    } else if (op == 4) {
        sim3_map(A[i], b + 3 * (size_t)i, out + 3 * (size_t)i);
    } else {
        ess_error(A[i], B[i], ((const Sim3d*)c)[i], out + 7 * (size_t)i);
    }
}

// orbgpu_unit_essgraph_stage: the upper triangle of H in system order out of the solver's storage
// (an element whose tile the block-sparse pattern does not hold is zero)
__global__ void __launch_bounds__(256) k_ess_dump_h(int n, EssAddr sa, double* out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    const int r = (int)(idx / n), c = (int)(idx % n);
    double v = 0;
    if (r <= c) {
        bool held = true;
        if (!sa.dense) {
            int a = sa.prow[r / 7] + r % 7, b = sa.prow[c / 7] + c % 7;
            if (a > b) {
                const int t = a;
                a = b;
                b = t;
            }
            held = sa.slot_of[(size_t)(a >> 6) * sa.nt + (b >> 6)] >= 0;
        }
        if (held) v = *sa.at(r, c);
    }
    out[idx] = v;
}

// ---------------------------------------------------------------- host
class EssGraphEngine {
public:
    ~EssGraphEngine() {
        if (arena_) (void)hipFree(arena_);
        if (hScal_) (void)hipHostFree(hScal_);
        if (stream_) (void)hipStreamDestroy(stream_);
    }
    int init() {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -4;
        ORB_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        ORB_HIP_CHECK(hipHostMalloc((void**)&hScal_, 16 * sizeof(double)));
        int dev = 0;
        ORB_HIP_CHECK(hipGetDevice(&dev));
        hipDeviceProp_t prop;
        ORB_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        ldsMax_ = prop.sharedMemPerBlock > 2048 ? prop.sharedMemPerBlock - 1024 : 0;
        return 0;
    }
    // stage == nullptr: the optimisation (R written).  Else the unit entry: one full pass and one
    // trial at stageLambda through the launches the LM loop uses, the intermediate buffers copied
    // into *stage; R and nIterations are not used.
    int run(const essgraph_problem* P, int nIterations, essgraph_result* R, essgraph_stage* stage = nullptr,
            double stageLambda = 0);

private:
    hipStream_t stream_ = nullptr;
    void* arena_ = nullptr;
    size_t cap_ = 0;
    double* hScal_ = nullptr;   // pinned
    size_t ldsMax_ = 0;
    SparseLdlt sp_;
};

static inline int ess_nblk(int n, int b) { return (n + b - 1) / b; }

// rows the dense solver takes (orbgpu_unit_set_ess_dense_max lowers it so tests put a small
// system through the block-sparse solver)
static std::atomic<int> g_ess_dense_max{kDenseMaxN};
int debug_set_ess_dense_max(int rows) {
    if (rows < 0 || rows > kDenseMaxN) return 1;
    g_ess_dense_max.store(rows);
    return 0;
}

int EssGraphEngine::run(const essgraph_problem* P, int nIterations, essgraph_result* R, essgraph_stage* stage,
                        double stageLambda) {
    hipStream_t s = stream_;
    const int nKF = P->nKF, nE = P->nE, nMP = stage ? 0 : P->nMP;   // the stage entry moves no map points
    const int fix = P->bFixScale ? 1 : 0;
    if (ess_nblk(nE, 64) > kEssSumMaxChunks) return -3;
    // ---- system vertices: free with at least one edge, in the caller's order
    std::vector<int> sysIdx(nKF, -1);
    std::vector<uint8_t> hasEdge(nKF, 0);
    for (int e = 0; e < nE; e++) hasEdge[P->edge_i[e]] = hasEdge[P->edge_j[e]] = 1;
    int nV = 0;
    for (int v = 0; v < nKF; v++)
        if (!P->fixed[v] && hasEdge[v]) sysIdx[v] = nV++;
    const int n = 7 * nV;
    if (ess_nblk(n, 64) > kEssSumMaxChunks) return -3;
    // ---- gather lists: key (a, b), a <= b in system order; entries in edge order
    struct Ent {
        int64_t key;
        int ent;
    };
    std::vector<Ent> ents;
    ents.reserve(3 * (size_t)nE);
    for (int e = 0; e < nE; e++) {
        const int a = sysIdx[P->edge_i[e]], b = sysIdx[P->edge_j[e]];
        if (a >= 0) ents.push_back({(int64_t)a * nV + a, 2 * e});
        if (b >= 0) ents.push_back({(int64_t)b * nV + b, 2 * e + 1});
        if (a >= 0 && b >= 0) {
            if (a < b) ents.push_back({(int64_t)a * nV + b, 2 * e});
            else ents.push_back({(int64_t)b * nV + a, 2 * e + 1});
        }
    }
    std::stable_sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) { return x.key < y.key; });
    std::vector<int> blkStart, blkA, blkB, entList(ents.size());
    for (size_t q = 0; q < ents.size(); q++) {
        entList[q] = ents[q].ent;
        if (q == 0 || ents[q].key != ents[q - 1].key) {
            blkStart.push_back((int)q);
            blkA.push_back((int)(ents[q].key / nV));
            blkB.push_back((int)(ents[q].key % nV));
        }
    }
    const int nBlk = (int)blkA.size();
    blkStart.push_back((int)ents.size());
    // ---- solver of this call
    const bool optimise = (stage || nIterations > 0) && nE > 0 && nV > 0;
    DensePlan dense;
    bool tiled = false;
    if (optimise) {
        if (n <= g_ess_dense_max.load()) dense = dense_ldlt_plan(n, ldsMax_);
        if (dense.kernel == DenseKernel::None) {
            std::vector<int> adjStart(nV + 1, 0), adj;
            std::vector<std::vector<int>> nb(nV);
            for (int k = 0; k < nBlk; k++)
                if (blkA[k] != blkB[k]) {
                    nb[blkA[k]].push_back(blkB[k]);
                    nb[blkB[k]].push_back(blkA[k]);
                }
            for (int v = 0; v < nV; v++) {
                std::sort(nb[v].begin(), nb[v].end());
                adjStart[v] = (int)adj.size();
                adj.insert(adj.end(), nb[v].begin(), nb[v].end());
            }
            adjStart[nV] = (int)adj.size();
            if (int e = sp_.build(n, 7, adjStart, adj, /*nd=*/true, s)) return e == -3 ? -3 : -2;
            tiled = true;
        }
    }
    // ---- arena
    const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t off = 0;
    const auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += al(std::max<size_t>(bytes, 8));
        return o;
    };
    const size_t oScw = carve(sizeof(Sim3d) * nKF), oSnc = carve(sizeof(Sim3d) * nKF);
    const size_t oFixed = carve(nKF), oSys = carve(sizeof(int) * nKF);
    const size_t oEi = carve(sizeof(int32_t) * nE), oEj = carve(sizeof(int32_t) * nE), oLoop = carve(nE);
    const size_t oBlkS = carve(sizeof(int) * (nBlk + 1)), oBlkA = carve(sizeof(int) * nBlk);
    const size_t oBlkB = carve(sizeof(int) * nBlk), oEnt = carve(sizeof(int) * entList.size());
    const size_t oRef = carve(sizeof(int32_t) * nMP), oPos = carve(sizeof(float) * 3 * nMP);
    const size_t inBytes = off;   // everything above is uploaded
    const size_t oEst = carve(sizeof(Sim3d) * nKF), oBak = carve(sizeof(Sim3d) * nKF), oSwc = carve(sizeof(Sim3d) * nKF);
    const size_t oMeas = carve(sizeof(Sim3d) * nE), oErr = carve(sizeof(double) * 7 * nE);
    const size_t oChi = carve(sizeof(double) * nE), oJ = carve(sizeof(double) * kEssJ * nE);
    const size_t oB = carve(sizeof(double) * n), oX = carve(sizeof(double) * n), oScal = carve(sizeof(double) * 16);
    const size_t oS = carve(optimise && !tiled ? sizeof(double) * (size_t)n * n : 8), oTcw = carve(sizeof(float) * 16 * nKF);
    const size_t oH = carve(stage && stage->H && optimise ? sizeof(double) * (size_t)n * n : 8);   // the stage entry's copy of H
    if (off > cap_) {
        if (arena_) (void)hipFree(arena_);
        arena_ = nullptr;
        cap_ = 0;
        ORB_HIP_CHECK(hipMalloc(&arena_, off));
        cap_ = off;
    }
    char* d = (char*)arena_;
    std::vector<char> h(inBytes, 0);
    std::memcpy(h.data() + oScw, P->Scw, sizeof(Sim3d) * nKF);
    std::memcpy(h.data() + oSnc, P->ScwNonCorrected, sizeof(Sim3d) * nKF);
    std::memcpy(h.data() + oFixed, P->fixed, nKF);
    std::memcpy(h.data() + oSys, sysIdx.data(), sizeof(int) * nKF);
    if (nE) {
        std::memcpy(h.data() + oEi, P->edge_i, sizeof(int32_t) * nE);
        std::memcpy(h.data() + oEj, P->edge_j, sizeof(int32_t) * nE);
        std::memcpy(h.data() + oLoop, P->edge_loop, nE);
    }
    std::memcpy(h.data() + oBlkS, blkStart.data(), sizeof(int) * (nBlk + 1));
    if (nBlk) {
        std::memcpy(h.data() + oBlkA, blkA.data(), sizeof(int) * nBlk);
        std::memcpy(h.data() + oBlkB, blkB.data(), sizeof(int) * nBlk);
        std::memcpy(h.data() + oEnt, entList.data(), sizeof(int) * entList.size());
    }
    if (nMP) {
        std::memcpy(h.data() + oRef, P->mp_ref, sizeof(int32_t) * nMP);
        std::memcpy(h.data() + oPos, P->mp_pos, sizeof(float) * 3 * nMP);
    }
    ORB_HIP_CHECK(hipMemcpyAsync(d, h.data(), inBytes, hipMemcpyHostToDevice, s));
    ORB_HIP_CHECK(hipMemcpyAsync(d + oEst, d + oScw, sizeof(Sim3d) * nKF, hipMemcpyDeviceToDevice, s));
    Sim3d* dEst = (Sim3d*)(d + oEst);
    Sim3d* dBak = (Sim3d*)(d + oBak);
    const Sim3d* dScw = (const Sim3d*)(d + oScw);
    double *dB = (double*)(d + oB), *dX = (double*)(d + oX), *dScal = (double*)(d + oScal), *dS = (double*)(d + oS);
    double* dChi = (double*)(d + oChi);
    const int* dSys = (const int*)(d + oSys);
    ORB_HIP_CHECK(hipMemsetAsync(dScal, 0, 16 * sizeof(double), s));
    if (n) ORB_HIP_CHECK(hipMemsetAsync(dX, 0, sizeof(double) * n, s));
    const EssDev E{nKF, nE, fix, dEst, (const Sim3d*)(d + oMeas), (const int32_t*)(d + oEi), (const int32_t*)(d + oEj),
                   (const uint8_t*)(d + oFixed), (double*)(d + oErr), dChi, (double*)(d + oJ)};
    const auto sum_shm = [](int k) {
        const int m = std::max(1, ess_nblk(k, 64));
        return sizeof(double) * (size_t)(m + ess_nblk(m, 64));
    };
    const size_t shmE = sum_shm(nE), shmN = sum_shm(n);
    const auto lin = [&](int full, double* out) {
        hipLaunchKernelGGL(k_ess_lin, dim3(ess_nblk(nE, kEssEdgesPerBlock)), dim3(256), 0, s, E, full);
        hipLaunchKernelGGL(k_ess_sum, dim3(1), dim3(kEssSumThreads), shmE, s, 0, nE, (const double*)dChi, (const double*)nullptr, 0.0,
                           out);
    };
    const auto read_scal = [&]() -> int {
        ORB_HIP_CHECK(hipGetLastError());
        ORB_HIP_CHECK(hipMemcpyAsync(hScal_, dScal, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
        ORB_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    };
    if (R) R->n_solves = R->lm_trials = 0;
    int nTrace = 0;
    const auto trace = [&](double c) {
        if (R && nTrace < R->trace_cap) R->chi2[nTrace] = c;
        nTrace++;
    };
    // the stage entry's device-to-host copies (a NULL destination is skipped)
    const auto fetch = [&](void* dst, const void* src, size_t bytes) -> int {
        if (dst && bytes) ORB_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        return 0;
    };
    // ---- measurements and the initial chi2
    if (nE) {
        hipLaunchKernelGGL(k_ess_meas, dim3(ess_nblk(nE, 256)), dim3(256), 0, s, nE, E.ei, E.ej,
                           (const uint8_t*)(d + oLoop), dScw, (const Sim3d*)(d + oSnc), (Sim3d*)(d + oMeas));
        lin(0, dScal + 0);
    }
    if (int e = read_scal()) return e;
    trace(hScal_[0]);
    // ---- OptimizationAlgorithmLevenberg, setUserLambdaInit(1e-16), optimize(nIterations)
    if (optimise) {
        const EssAddr sa = tiled ? EssAddr{nullptr, n, sp_.addr().slot_of, sp_.addr().tiles, sp_.addr().nt, sp_.addr().prow}
                                 : EssAddr{dS, n, nullptr, nullptr, 0, nullptr};
        // one LM trial in three steps, shared by the loop below and the stage entry
        const auto assemble = [&](double lambda) -> int {
            if (tiled) {
                if (int e = sp_.zero(s)) return e;
            } else {
                ORB_HIP_CHECK(hipMemsetAsync(dS, 0, sizeof(double) * (size_t)n * n, s));
            }
            hipLaunchKernelGGL(k_ess_assemble, dim3(nBlk), dim3(64), 0, s, (const int*)(d + oBlkS),
                               (const int*)(d + oBlkA), (const int*)(d + oBlkB), (const int*)(d + oEnt),
                               (const double*)E.J, (const double*)E.err, lambda, sa, dB);
            return 0;
        };
        const auto solve = [&]() -> int {
            if (tiled) return sp_.solve(dB, dX, dScal, s);
            dense_ldlt_launch(dense, n, dS, dB, dX, dScal, nullptr, s);
            return 0;
        };
        const auto update_and_evaluate = [&](double lambda) -> int {
            hipLaunchKernelGGL(k_ess_update, dim3(ess_nblk(nKF, 256)), dim3(256), 0, s, nKF, fix, dSys, dEst, dBak, dX);
            lin(0, dScal + 1);
            hipLaunchKernelGGL(k_ess_sum, dim3(1), dim3(kEssSumThreads), shmN, s, 1, n, (const double*)dX, (const double*)dB, lambda,
                               dScal + 2);
            return read_scal();
        };
        if (stage) {
            lin(1, dScal + 0);
            if (fetch(stage->err, E.err, sizeof(double) * 7 * nE) || fetch(stage->chi2e, dChi, sizeof(double) * nE) ||
                fetch(stage->J, E.J, sizeof(double) * kEssJ * nE))
                return -2;
            if (int e = assemble(stageLambda)) return e;
            if (stage->H) {
                double* dH = (double*)(d + oH);
                hipLaunchKernelGGL(k_ess_dump_h, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, s, n, sa, dH);
                if (fetch(stage->H, dH, sizeof(double) * (size_t)n * n)) return -2;
            }
            if (fetch(stage->b, dB, sizeof(double) * n)) return -2;
            if (int e = solve()) return e;
            if (fetch(stage->x_solve, dX, sizeof(double) * n)) return -2;
            if (int e = update_and_evaluate(stageLambda)) return e;
            if (fetch(stage->x, dX, sizeof(double) * n) || fetch(stage->est_trial, dEst, sizeof(Sim3d) * nKF) ||
                fetch(stage->chi2e_trial, dChi, sizeof(double) * nE))
                return -2;
            ORB_HIP_CHECK(hipStreamSynchronize(s));
            stage->solver = tiled ? 1 : 0;
            stage->ok = hScal_[3] != 0.0;
            stage->chi2 = hScal_[0];
            stage->chi2_trial = hScal_[1];
            stage->scale = hScal_[2];
        }
        double lambda = 1e-16, ni = 2;
        int nBad = 0;
        bool term = stage != nullptr;
        for (int it = 0; it < nIterations && !term; it++) {
            lin(1, dScal + 0);
            double currentChi = 0, iniChi = 0, rho = 0;
            bool haveChi = false;
            int qmax = 0;
            do {
                if (int e = assemble(lambda)) return e;
                if (int e = solve()) return e;
                if (int e = update_and_evaluate(lambda)) return e;
                if (!haveChi) {
                    currentChi = iniChi = hScal_[0];
                    haveChi = true;
                }
                bool accepted = false;
                double tempChi = 0;
                rho = lm_decide(hScal_[3] != 0.0, hScal_[1], hScal_[2], &lambda, &ni, &currentChi, &accepted, &tempChi);
                if (!accepted)
                    ORB_HIP_CHECK(hipMemcpyAsync(dEst, dBak, sizeof(Sim3d) * nKF, hipMemcpyDeviceToDevice, s));
                qmax++;
                R->lm_trials++;
            } while (rho < 0 && qmax < 10);
            R->n_solves++;
            trace(currentChi);
            term = lm_terminate(qmax, rho, iniChi, currentChi, &nBad);
        }
    }
    if (stage) {
        if (!optimise) {   // nothing to solve: the full pass alone
            if (nE) {
                lin(1, dScal + 0);
                if (fetch(stage->err, E.err, sizeof(double) * 7 * nE) || fetch(stage->chi2e, dChi, sizeof(double) * nE) ||
                    fetch(stage->J, E.J, sizeof(double) * kEssJ * nE))
                    return -2;
            }
            stage->solver = -1;
            stage->ok = 0;
            stage->chi2 = hScal_[0];
            stage->chi2_trial = stage->scale = 0;
        }
        stage->nV = nV;
        if (stage->sysIdx) std::copy(sysIdx.begin(), sysIdx.end(), stage->sysIdx);
        if (fetch(stage->meas, E.meas, sizeof(Sim3d) * nE)) return -2;
        ORB_HIP_CHECK(hipGetLastError());
        ORB_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    // ---- write-back
    hipLaunchKernelGGL(k_ess_finish, dim3(ess_nblk(nKF, 256)), dim3(256), 0, s, nKF, (const Sim3d*)dEst,
                       (Sim3d*)(d + oSwc), (float*)(d + oTcw));
    if (nMP)
        hipLaunchKernelGGL(k_ess_points, dim3(ess_nblk(nMP, 256)), dim3(256), 0, s, nMP, (const int32_t*)(d + oRef), dScw,
                           (const Sim3d*)(d + oSwc), (float*)(d + oPos));
    ORB_HIP_CHECK(hipGetLastError());
    ORB_HIP_CHECK(hipMemcpyAsync(R->Scw, dEst, sizeof(Sim3d) * nKF, hipMemcpyDeviceToHost, s));
    ORB_HIP_CHECK(hipMemcpyAsync(R->Tcw, d + oTcw, sizeof(float) * 16 * nKF, hipMemcpyDeviceToHost, s));
    if (nMP) ORB_HIP_CHECK(hipMemcpyAsync(R->mp_pos, d + oPos, sizeof(float) * 3 * nMP, hipMemcpyDeviceToHost, s));
    ORB_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

static EssGraphEngine* ess_engine(int* rc) {
    thread_local EssGraphEngine* e = nullptr;
    thread_local int erc = 0;
    if (!e) {
        e = new EssGraphEngine();
        erc = e->init();
    }
    *rc = erc;
    return e;
}

int essgraph_run(const essgraph_problem* P, int nIterations, essgraph_result* R) {
    int erc = 0;
    EssGraphEngine* e = ess_engine(&erc);
    if (erc) return erc;
    return e->run(P, nIterations, R);
}

int essgraph_stage_run(const essgraph_problem* P, double lambda, essgraph_stage* out) {
    int erc = 0;
    EssGraphEngine* e = ess_engine(&erc);
    if (erc) return erc;
    return e->run(P, 0, nullptr, out, lambda);
}

int essgraph_unit_sim3(int op, int n, const double* a, const double* b, const double* c, double* out) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return -4;
    if (n == 0) return 0;
    const size_t inA = op == 0 ? 7 : 8, inB = op == 2 || op == 5 ? 8 : op == 4 ? 3 : 0, inC = op == 5 ? 8 : 0;
    const size_t nOut = op == 1 || op == 5 ? 7 : op == 4 ? 3 : 8;
    const size_t per = inA + inB + inC + nOut;
    double* dm = nullptr;
    ORB_HIP_CHECK(hipMalloc((void**)&dm, sizeof(double) * per * n));
    double *dA = dm, *dB = dA + inA * n, *dC = dB + inB * n, *dO = dC + inC * n;
    int rc = 0;
    const auto up = [&](double* dst, const double* src, size_t k) {
        if (k && !rc && hipMemcpy(dst, src, sizeof(double) * k * n, hipMemcpyHostToDevice) != hipSuccess) rc = -2;
    };
    up(dA, a, inA);
    up(dB, b, inB);
    up(dC, c, inC);
    if (!rc) {
        hipLaunchKernelGGL(k_unit_sim3, dim3(ess_nblk(n, 256)), dim3(256), 0, 0, op, n, (const double*)dA,
                           (const double*)dB, (const double*)dC, dO);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, dO, sizeof(double) * nOut * n, hipMemcpyDeviceToHost) != hipSuccess)
            rc = -2;
    }
    (void)hipFree(dm);
    return rc;
}

}  // namespace orbgpu
