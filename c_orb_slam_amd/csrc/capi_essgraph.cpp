// capi_essgraph.cpp -- extern "C" Optimizer_OptimizeEssentialGraph (include/orbslam_gpu.h).
// Replaces Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:781-1044).
#include <cmath>

#include "essgraph.hpp"

namespace {
bool sim3_rows_ok(const double* S, int n) {
    for (int v = 0; v < n; v++) {
        for (int k = 0; k < 8; k++)
            if (!std::isfinite(S[8 * (size_t)v + k])) return false;
        if (!(S[8 * (size_t)v + 7] > 0)) return false;
    }
    return true;
}
// the whole problem is checked before the device is touched
bool problem_ok(const essgraph_problem* P) {
    if (!P) return false;
    if (P->nKF <= 0 || P->nE < 0 || P->nMP < 0) return false;
    if (!P->Scw || !P->ScwNonCorrected || !P->fixed) return false;
    if (P->nE > 0 && (!P->edge_i || !P->edge_j || !P->edge_loop)) return false;
    if (P->nMP > 0 && (!P->mp_pos || !P->mp_ref)) return false;
    if (!sim3_rows_ok(P->Scw, P->nKF) || !sim3_rows_ok(P->ScwNonCorrected, P->nKF)) return false;
    for (int e = 0; e < P->nE; e++) {
        const int i = P->edge_i[e], j = P->edge_j[e];
        if (i < 0 || i >= P->nKF || j < 0 || j >= P->nKF || i == j) return false;
    }
    for (int p = 0; p < P->nMP; p++) {
        if (P->mp_ref[p] < -1 || P->mp_ref[p] >= P->nKF) return false;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(P->mp_pos[3 * (size_t)p + k])) return false;
    }
    return true;
}
int abi_code(int r) {
    if (r == -4) return ORB_E_NODEVICE;
    if (r == -3) return ORB_E_CAPACITY;
    return r ? ORB_E_HIP : ORB_OK;
}
}  // namespace

extern "C" int Optimizer_OptimizeEssentialGraph(const essgraph_problem* P, int nIterations, essgraph_result* R) {
    if (!R || nIterations < 0 || !problem_ok(P)) return ORB_E_INVALID;
    if (P->nMP > 0 && !R->mp_pos) return ORB_E_INVALID;
    if (!R->Scw || !R->Tcw || R->trace_cap < 0 || (R->trace_cap > 0 && !R->chi2)) return ORB_E_INVALID;
    return abi_code(orbgpu::essgraph_run(P, nIterations, R));
}

extern "C" int orbgpu_unit_essgraph_stage(const essgraph_problem* P, double lambda, essgraph_stage* out) {
    if (!out || !std::isfinite(lambda) || lambda < 0 || !problem_ok(P)) return ORB_E_INVALID;
    return abi_code(orbgpu::essgraph_stage_run(P, lambda, out));
}

extern "C" int orbgpu_unit_sim3(int op, int n, const double* a, const double* b, const double* c, double* out) {
    if (op < 0 || op > 5 || n < 0) return ORB_E_INVALID;
    if (n > 0 && (!a || !out || ((op == 2 || op == 4 || op == 5) && !b) || (op == 5 && !c))) return ORB_E_INVALID;
    return abi_code(orbgpu::essgraph_unit_sim3(op, n, a, b, c, out));
}

extern "C" int orbgpu_unit_set_ess_dense_max(int rows) {
    return orbgpu::debug_set_ess_dense_max(rows) ? ORB_E_INVALID : ORB_OK;
}
