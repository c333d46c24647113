// essgraph.hpp -- gfx950 Optimizer::OptimizeEssentialGraph (see essgraph.hip)
#pragma once
#include "../../include/orbslam_gpu.h"

namespace orbgpu {

// 0, or -2 (HIP error), -3 (capacity), -4 (no device).  P is validated by the caller (capi_essgraph.cpp).
int essgraph_run(const essgraph_problem* P, int nIterations, essgraph_result* R);

}  // namespace orbgpu
