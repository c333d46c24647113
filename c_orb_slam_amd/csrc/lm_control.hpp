// lm_control.hpp -- the accept / reject arithmetic of g2o's OptimizationAlgorithmLevenberg::solve
// (optimization_algorithm_levenberg.cpp:100-140), shared by the host-driven LM loops
// (BaEngine::lm_solve, EssGraphEngine::run).  Plain IEEE host arithmetic in the reference's
// order, so every caller takes the same decision from the same scalars.
#pragma once
#include <cfloat>
#include <cmath>

namespace orbgpu {

// One trial's decision.  ok: the factorisation succeeded; tempChi: the trial's chi2; scale:
// computeScale()'s x^T (lambda x + b), without the 1e-3.  Returns rho; on acceptance (*accepted)
// lambda, ni and currentChi take the new values, otherwise lambda and ni grow and the caller
// restores the estimates.  *tempChiOut: the chi2 the decision used (DBL_MAX after a failed solve).
inline double lm_decide(bool ok, double tempChi, double scale, double* lambda, double* ni, double* currentChi,
                        bool* accepted, double* tempChiOut) {
    if (!ok) tempChi = DBL_MAX;
    double rho = *currentChi - tempChi;
    scale += 1e-3;
    rho /= scale;
    if (rho > 0 && std::isfinite(tempChi)) {
        const double a3 = 2 * rho - 1;
        double alpha = 1. - (a3 * a3) * a3;
        alpha = std::fmin(alpha, 2. / 3.);
        const double scaleFactor = std::fmax(1. / 3., alpha);
        *lambda *= scaleFactor;
        *ni = 2;
        *currentChi = tempChi;
        *accepted = true;
    } else {
        *lambda *= *ni;
        *ni *= 2;
        *accepted = false;
    }
    *tempChiOut = tempChi;
    return rho;
}

// After the trials of one iteration (qmax of them, the last with rho): true when the optimiser
// terminates -- 10 trials, rho == 0, or the third iteration in a row that gained less than 1e-3
// of its initial chi2 (nBad).
inline bool lm_terminate(int qmax, double rho, double iniChi, double currentChi, int* nBad) {
    if (qmax == 10 || rho == 0) return true;
    if ((iniChi - currentChi) * 1e3 < iniChi) (*nBad)++;
    else *nBad = 0;
    return *nBad >= 3;
}

}  // namespace orbgpu
