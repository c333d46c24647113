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
}  // namespace

extern "C" int Optimizer_OptimizeEssentialGraph(const essgraph_problem* P, int nIterations, essgraph_result* R) {
    // the whole problem is checked before the device is touched
    if (!P || !R || nIterations < 0) return ORB_E_INVALID;
    if (P->nKF <= 0 || P->nE < 0 || P->nMP < 0) return ORB_E_INVALID;
    if (!P->Scw || !P->ScwNonCorrected || !P->fixed) return ORB_E_INVALID;
    if (P->nE > 0 && (!P->edge_i || !P->edge_j || !P->edge_loop)) return ORB_E_INVALID;
    if (P->nMP > 0 && (!P->mp_pos || !P->mp_ref || !R->mp_pos)) return ORB_E_INVALID;
    if (!R->Scw || !R->Tcw || R->trace_cap < 0 || (R->trace_cap > 0 && !R->chi2)) return ORB_E_INVALID;
    if (!sim3_rows_ok(P->Scw, P->nKF) || !sim3_rows_ok(P->ScwNonCorrected, P->nKF)) return ORB_E_INVALID;
    for (int e = 0; e < P->nE; e++) {
        const int i = P->edge_i[e], j = P->edge_j[e];
        if (i < 0 || i >= P->nKF || j < 0 || j >= P->nKF || i == j) return ORB_E_INVALID;
    }
    for (int p = 0; p < P->nMP; p++) {
        if (P->mp_ref[p] < -1 || P->mp_ref[p] >= P->nKF) return ORB_E_INVALID;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(P->mp_pos[3 * (size_t)p + k])) return ORB_E_INVALID;
    }
    const int r = orbgpu::essgraph_run(P, nIterations, R);
    if (r == -4) return ORB_E_NODEVICE;
    if (r == -3) return ORB_E_CAPACITY;
    return r ? ORB_E_HIP : ORB_OK;
}
