// frame_input.hpp -- gfx950 frame input of the RGB-D sensor path (see frame_input.hip):
// Tracking::GrabImage*'s cvtColor and Frame::ComputeStereoFromRGBD with GrabImageRGBD's depth
// conversion.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "orb_extract.hpp"

namespace orbgpu {

// cv::cvtColor(im, im, CV_{RGB,BGR,RGBA,BGRA}2GRAY) over a batch of equal-sized device images in
// one launch: image b at src + b * img_stride (rows `step` bytes apart, `channels` = 3 or 4 bytes
// per pixel), grey image b at gray + b * gray_stride (rows gray_step bytes apart).  Any alignment.
int cvt_gray_launch(const uint8_t* src, int batch, int width, int height, int channels, int rgb, int step,
                    size_t img_stride, uint8_t* gray, int gray_step, size_t gray_stride, hipStream_t s);
// widest image the launch's grid holds (quads of one image / 256 in grid.x, the batch in grid.y)
constexpr long long kCvtMaxQuads = 256LL * 0x7fffffff;
constexpr int kCvtMaxBatch = 65535;

// cv::remap(src, dst, map1, map2, INTER_LINEAR) (Extractor::set_remap / remap): largest source and
// destination side, the record value of a pixel whose taps are all outside any source, and the
// images of one slot a thread makes from the record it holds (4 measured fastest of 1, 2, 4, 8 and
// 64 at 128 images of 752x480; ORBGPU_REMAP_IPT overrides it for that measurement)
constexpr int kRemapMaxDim = 16384;
constexpr uint32_t kRemapOutside = 0xFFFFu;
constexpr int kRemapImagesPerThread = 4;

constexpr int kDepthU16 = 0, kDepthF32 = 1;   // ORB_DEPTH_U16 / ORB_DEPTH_F32

// Frame::ComputeStereoFromRGBD of one frame; every pointer is device memory
struct RgbdDev {
    int N, type;                // keypoints; kDepthU16 / kDepthF32
    int cols, rows;
    int convert;                // GrabImageRGBD's gate: the pixel is multiplied by `factor`
    float factor, mbf;
    size_t step;                // bytes per depth row
    const orb_kp_dev* keys;     // mvKeys
    const orb_kp_dev* keysUn;   // mvKeysUn
    const uint8_t* depth;       // imD
    float* uRight;              // out: mvuRight (N)
    float* depthOut;            // out: mvDepth (N)
    int* count;                 // out: keypoints with depth (zeroed before the launch)
};
constexpr int kRgbdPerLaunch = 44;   // frames per launch, passed by value (kernel-argument space)
// enqueue on `s` (no staging buffer: the frames are kernel arguments)
int rgbd_batch(const RgbdDev* probs, int count, hipStream_t s);

}  // namespace orbgpu
