// loopcorrect.hpp -- gfx950 LoopClosing map correction over the Map handle's relation: the first
// half of LoopClosing::CorrectLoop and the write-back of LoopClosing::RunGlobalBundleAdjustment
// (reference src/LoopClosing.cc).  Kernels in loopcorrect.hip, the C entries in
// capi_loopcorrect.cpp.  Every pointer below is a device pointer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "map.hpp"

namespace orbgpu {

constexpr int kLoopClaimIdleByte = 0x7f;   // the claim words idle at 0x7f7f7f7f, above every index

struct LoopCorrectDev {
    MapView V;
    int nkf;                   // listed keyframes, in processing order (ascending id)
    int cur;                   // processing index of the current keyframe
    const int32_t* kf_id;      // nkf
    const int32_t* kf_slot;    // nkf: the handle's slot of each
    const double* Scw;         // 8
    const float* scale;        // nlevels
    int nlevels;
    int n_kf_rows, n_pt_rows;
    float* Tcw;                // n_kf_rows x 16
    float* pos;
    float* normal;
    float* max_dist;
    float* min_dist;
    const uint8_t* bad;        // or null
    const int32_t* ref_kf;
    int32_t* corrected_ref;
    // work area of the call
    int32_t* proc;             // n_kf_rows, 0xff-filled: processing index of a listed id, else -1
    int32_t* claim;            // n_pt_rows, idle-filled: lowest processing index that holds the point
    double* corr;              // nkf x 8: CorrectedSim3 (Sim3d)
    double* noncorr;           // nkf x 8: NonCorrectedSim3
    double* corr_inv;          // nkf x 8
    float* newT;               // nkf x 16: the SetPose argument
    float* newOw;              // nkf x 3: its camera centre
    int32_t* counts;           // zeroed: n_corrected, n_ref_missing
};
// max_row = the longest listed row.  Queues the four kernels on s.
int loop_correct_launch(const LoopCorrectDev& D, int max_row, hipStream_t s);

struct GbaApplyDev {
    int n_kf_rows, n_pt_rows;
    float* Tcw;
    float* TcwGBA;
    float* TcwBef;             // or null
    const uint8_t* reached;    // n_kf_rows
    const int32_t* pair;       // (child, parent) ids, grouped by level
    float* pos;
    const float* posGBA;
    const uint8_t* mp_in_gba;
    const uint8_t* bad;        // or null
    const int32_t* ref_kf;
    int32_t* counts;           // zeroed: n_mp_gba, n_mp_moved
};
// level_off[l] .. level_off[l + 1]: the pairs of dependent step l (nlevels + 1 offsets).
int gba_apply_launch(const GbaApplyDev& D, int nlevels, const int* level_off, hipStream_t s);

}  // namespace orbgpu
