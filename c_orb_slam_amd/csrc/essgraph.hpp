// essgraph.hpp -- gfx950 Optimizer::OptimizeEssentialGraph (see essgraph.hip)
#pragma once
#include "../../include/orbslam_gpu.h"

namespace orbgpu {

// 0, or -2 (HIP error), -3 (capacity), -4 (no device).  P is validated by the caller (capi_essgraph.cpp).
int essgraph_run(const essgraph_problem* P, int nIterations, essgraph_result* R);

// Unit entries (include/orbslam_gpu.h orbgpu_unit_essgraph_stage, orbgpu_unit_sim3,
// orbgpu_unit_set_ess_dense_max): same return codes; the knob returns 1 on a value out of range.
int essgraph_stage_run(const essgraph_problem* P, double lambda, essgraph_stage* out);
int essgraph_unit_sim3(int op, int n, const double* a, const double* b, const double* c, double* out);
int debug_set_ess_dense_max(int rows);

}  // namespace orbgpu
