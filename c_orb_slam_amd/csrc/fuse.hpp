// fuse.hpp -- gfx950 LocalMapping::SearchInNeighbors (see fuse.hip): the projection of every
// (target keyframe, map point) pair, the per-pass ORBmatcher::Fuse selection and the scatter of
// recomputed descriptors.  Reference src/LocalMapping.cc:454-553, src/ORBmatcher.cc:825-975.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "orb_extract.hpp"

namespace orbgpu {

// one keyframe a pass fuses into (device pointers; the grid is Matcher::build_grids')
struct FuseKF {
    float R[9], t[3], O[3];   // Rcw, tcw, Ow = -Rcw^T * tcw
    float fx, fy, cx, cy, bf;
    float minX, maxX, minY, maxY, gridWInv, gridHInv;
    int N, nlevels;
    const orb_kp_dev* keys;
    const uint8_t* desc;
    const float* uRight;      // null: monocular keyframe
    const int* gridStart;     // kGridCells + 1
    const int* gridIdx;       // N
    const float* scale;       // nlevels
};

// the projection of `npts` listed points into `ntargets` keyframes: pair (t, i) at t * npts + i
struct FuseProjDev {
    const FuseKF* kf;
    const int32_t* kf_of;     // ntargets: target -> index into kf
    int ntargets, npts;
    const int32_t* pts;       // npts: map-point ids, -1 = none
    int n_table;
    const float* pos;         // the map-point table (rows = ids)
    const float* normal;
    const float* max_dist;
    const float* min_dist;
    float logScaleFactor, th;
    float4* uvr;              // out: u, v, ur, radius
    int32_t* level;           // out: nPredictedLevel, -1 = rejected
};

// one Fuse pass into keyframe kf[k] over the listed points
struct FuseMatchDev {
    const FuseKF* kf;
    int k, npts;
    const int32_t* pts;
    const uint8_t* skip;      // npts: !pMP || isBad() || IsInKeyFrame(pKF) when the pass starts
    const uint8_t* desc;      // the working descriptor table (rows = ids)
    const float4* uvr;        // this pass's slice of the projection
    const int32_t* level;
    int32_t* best;            // out npts: bestIdx with bestDist <= TH_LOW, else -1
};

// Device buffers and timing events of the call, kept on the Map handle between calls.
struct FuseWork {
    static constexpr int kBufs = 4;   // keyframes + table + forward pass | backward pass | gathers | results
    void* buf[kBufs] = {};
    size_t cap[kBufs] = {};
    std::vector<hipEvent_t> ev;
    float ms[5] = {-1.f, -1.f, -1.f, -1.f, -1.f};
    bool timed = false;
    ~FuseWork();
    // at least `bytes` of buffer i; growing waits for `s` first.  null: out of memory
    void* get(int i, size_t bytes, hipStream_t s);
    // event k of this call (created on first use); null on failure
    hipEvent_t event(size_t k);
};

// LoopClosing_SearchAndFuse's state on the Map handle: the device buffers and events, and two pinned
// host blocks (0: the staged upload of a call, 1: a pass's skip bytes and best[]).
struct LoopFuseWork {
    FuseWork dev;
    void* pin[2] = {};
    size_t pin_cap[2] = {};
    ~LoopFuseWork();
    // at least `bytes` of pinned block i; growing waits for `s` first.  null: out of memory
    void* pinned(int i, size_t bytes, hipStream_t s);
};

int fuse_project_launch(const FuseProjDev& P, hipStream_t s);
int fuse_match_launch(const FuseMatchDev& M, hipStream_t s);
// The Sim3 form (ORBmatcher.cc:977-1100): kf[t] is target t (kf_of is not read), invz = 1.0 / z, no
// uRight; the match has no reprojection gate.
int fuse_project_sim3_launch(const FuseProjDev& P, hipStream_t s);
int fuse_match_sim3_launch(const FuseMatchDev& M, hipStream_t s);
// table[id[p]] = rows[start[p] + best[p]] for every p with best[p] >= 0 (32-byte rows)
int fuse_take_desc_launch(int npts, const int32_t* id, const int32_t* start, const int32_t* best,
                          const uint8_t* rows, uint8_t* table, hipStream_t s);

}  // namespace orbgpu
