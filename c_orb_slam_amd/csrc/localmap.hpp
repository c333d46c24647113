// localmap.hpp -- gfx950 LocalMapping::CreateNewMapPoints geometry and the MapPoint updates
// (see localmap.hip).  Reference src/LocalMapping.cc:207-452, src/MapPoint.cc:242-307, 331-371.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbgpu {

// One keyframe of a CreateNewMapPoints call: header 0 is the current keyframe, 1..count its
// neighbours.  tab: float offset (in the call's table block) of mvScaleFactors[nlevels]
// followed by mvLevelSigma2[nlevels].
struct TriKF {
    float T[12];   // Tcw rows 0..2
    float fx, fy, cx, cy, invfx, invfy, bf, b;
    int nlevels, tab;
};

// One pair of SearchForTriangulation, gathered on the host (ur < 0: monocular keypoint)
struct TriPair {
    float x1, y1, ur1, z1;   // kp1.pt, mvuRight[idx1], mvDepth[idx1]
    float x2, y2, ur2, z2;
    int oct1, oct2, nb, pad;   // nb: the neighbour's header (1..count)
};
static_assert(sizeof(TriPair) == 48, "staging layout");

struct TriBatch {
    const TriKF* kf;
    const float* tab;
    const TriPair* pairs;
    int npairs;
    float ratioFactor;   // 1.5f * mfScaleFactor
    float* x3D;          // out npairs x 3 (written for status > 0)
    float* normal;       // out npairs x 3
    float* maxDist;      // out npairs
    float* minDist;      // out npairs
    int8_t* status;      // out npairs
};
// one launch for the whole batch on `s`
int triangulate_launch(const TriBatch& B, hipStream_t s);

struct PointUpdateDev {
    int npts;
    const int* obsStart;       // npts + 1
    const uint8_t* obsDesc;    // total x 32 or null
    int* best;                 // out npts
    const float* pos;          // npts x 3 or null
    const float* obsOw;        // total x 3
    const float* refOw;        // npts x 3
    const float* refScale;     // npts
    const float* refScaleTop;  // npts
    float* normal;             // out npts x 3
    float* maxDist;
    float* minDist;
};
int point_update_launch(const PointUpdateDev& U, hipStream_t s);

}  // namespace orbgpu
