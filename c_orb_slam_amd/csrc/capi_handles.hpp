// capi_handles.hpp -- the opaque C handles of include/orbslam_gpu.h (shared by the capi_*.cpp units).
#pragma once
#include <mutex>

#include "fuse.hpp"
#include "map.hpp"
#include "orb_extract.hpp"
#include "orb_match.hpp"

struct ORBextractor_t {
    orbgpu::Extractor* ex;
};

struct ORBmatcher_t {
    orbgpu::Matcher* m;
};

struct Map_t {
    orbgpu::Map map;
    std::mutex mu;   // stands for Map::mMutexMap, KeyFrame::mMutexFeatures / mMutexConnections
    orbgpu::FuseWork fuse;   // LocalMapping_SearchInNeighbors' device buffers (capi_fuse.cpp)
    orbgpu::LoopFuseWork loopfuse;   // LoopClosing_SearchAndFuse's buffers (capi_loopfuse.cpp)
};
