// frame_input.hip -- the RGB-D sensor path's frame input on gfx950.
//
// k_cvt_gray   Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular's cvtColor
//              (mbRGB picks RGB2GRAY or BGR2GRAY, 4 channels RGBA2GRAY / BGRA2GRAY), OpenCV 3.2's
//              8-bit path: (R*4899 + G*9617 + B*1868 + 8192) >> 14 in integers, alpha ignored.
//              "Parity unpinned" like the other OpenCV call sites.
// k_rgbd       Frame::ComputeStereoFromRGBD with the imDepth.convertTo(CV_32F, mDepthMapFactor)
//              of GrabImageRGBD folded in: the float depth image is never written, every keypoint
//              converts the one pixel it reads.
#include <algorithm>
#include <cstring>

#include "frame_input.hpp"

namespace orbgpu {

// ------------------------------------------------------------------ cvtColor
// One thread per 4 grey pixels of a row (a "quad"); consecutive lanes take consecutive quads, so a
// wave reads 768 B (3 channels) or 1 KiB (4 channels) and writes 256 B, contiguous.  A full quad
// whose source is dword aligned is read as 3 / 4 dwords, and written as one dword when its
// destination is; everything else (the tail of a row, rows that start off a dword) goes bytewise.
template <int CH>
__global__ void __launch_bounds__(256) k_cvt_gray(const uint8_t* __restrict__ src, size_t img_stride, int step,
                                                  int W, long long quads, int Q, int rgb,
                                                  uint8_t* __restrict__ gray, int gstep, size_t gstride) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= quads) return;
    const int row = (int)(t / Q);
    const int x0 = 4 * (int)(t - (long long)row * Q);
    const uint8_t* s = src + (size_t)blockIdx.y * img_stride + (size_t)row * (size_t)step + (size_t)x0 * CH;
    uint8_t* d = gray + (size_t)blockIdx.y * gstride + (size_t)row * (size_t)gstep + (size_t)x0;
    const int n = min(4, W - x0);
    const int c0 = rgb ? 4899 : 1868, c2 = rgb ? 1868 : 4899;   // weight of the first / third byte
    uint32_t g[4] = {0, 0, 0, 0};
    if (n == 4 && ((uintptr_t)s & 3) == 0) {
        uint32_t w[CH];
#pragma unroll
        for (int k = 0; k < CH; k++) w[k] = ((const uint32_t*)s)[k];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int b = p * CH;
            const uint32_t v0 = (w[b >> 2] >> (8 * (b & 3))) & 255u;
            const uint32_t v1 = (w[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 255u;
            const uint32_t v2 = (w[(b + 2) >> 2] >> (8 * ((b + 2) & 3))) & 255u;
            g[p] = (v0 * c0 + v1 * 9617u + v2 * c2 + 8192u) >> 14;
        }
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++)
            if (p < n)
                g[p] = ((uint32_t)s[p * CH] * c0 + (uint32_t)s[p * CH + 1] * 9617u + (uint32_t)s[p * CH + 2] * c2 +
                        8192u) >> 14;
    }
    if (n == 4 && ((uintptr_t)d & 3) == 0) {
        *(uint32_t*)d = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++)
            if (p < n) d[p] = (uint8_t)g[p];
    }
}

int cvt_gray_launch(const uint8_t* src, int batch, int width, int height, int channels, int rgb, int step,
                    size_t img_stride, uint8_t* gray, int gray_step, size_t gray_stride, hipStream_t s) {
    if (batch <= 0 || width <= 0 || height <= 0) return 0;
    const int Q = (width + 3) / 4;
    const long long quads = (long long)Q * height;
    if (quads > kCvtMaxQuads || batch > kCvtMaxBatch || (channels != 3 && channels != 4)) return -1;
    const dim3 grid((unsigned)((quads + 255) / 256), (unsigned)batch);
    if (channels == 3)
        hipLaunchKernelGGL(k_cvt_gray<3>, grid, dim3(256), 0, s, src, img_stride, step, width, quads, Q, rgb, gray,
                           gray_step, gray_stride);
    else
        hipLaunchKernelGGL(k_cvt_gray<4>, grid, dim3(256), 0, s, src, img_stride, step, width, quads, Q, rgb, gray,
                           gray_step, gray_stride);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

// Host images take extract()'s route: the pinned block h_in_, one H2D copy into d_in_.  ev_[0] is
// recorded behind the copy, which is what the next user of h_in_ (here or extract()) waits for.
int Extractor::cvt_color(const uint8_t* src, int B, int W, int H, int channels, int rgb, int step,
                         size_t img_stride, bool src_on_device, uint8_t* gray, int gray_step, size_t gray_stride) {
    hipStream_t s = stream_;
    if (!src_on_device) {
        const size_t need = img_stride * (size_t)(B - 1) + (size_t)step * (size_t)(H - 1) + (size_t)W * channels;
        if (need > in_cap_) {
            if (d_in_) (void)hipFree(d_in_);
            d_in_ = nullptr;
            in_cap_ = 0;
            ORB_HIP_CHECK(hipMalloc(&d_in_, need));
            in_cap_ = need;
        }
        if (h_in_) ORB_HIP_CHECK(hipEventSynchronize(ev_[0]));
        if (need > h_in_cap_) {
            if (h_in_) (void)hipHostFree(h_in_);
            h_in_ = nullptr;
            h_in_cap_ = 0;
            ORB_HIP_CHECK(hipHostMalloc(&h_in_, need));
            h_in_cap_ = need;
        }
        std::memcpy(h_in_, src, need);
        ORB_HIP_CHECK(hipMemcpyAsync(d_in_, h_in_, need, hipMemcpyHostToDevice, s));
        ORB_HIP_CHECK(hipEventRecord(ev_[0], s));
        src = (const uint8_t*)d_in_;
    }
    return cvt_gray_launch(src, B, W, H, channels, rgb, step, img_stride, gray, gray_step, gray_stride, s);
}

// ------------------------------------------------------------ ComputeStereoFromRGBD
// 4 bytes at any address: one dword when aligned (a depth row pitch need not be a multiple of 4)
__device__ __forceinline__ uint32_t load_u32_any(const uint8_t* p) {
    if (((uintptr_t)p & 3) == 0) return *(const uint32_t*)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct RgbdBatch {
    RgbdDev p[kRgbdPerLaunch];
};
static_assert(sizeof(RgbdBatch) <= 4032, "kernel-argument space (as UnprojBatch in stereo.hip)");

// One thread per keypoint.  d = imDepth.at<float>(kp.pt.y, kp.pt.x) after the conversion gate
// (float(raw) * mDepthMapFactor, one rounding); d > 0: mvDepth = d, mvuRight = kpU.pt.x - mbf / d;
// otherwise both -1.  A keypoint whose truncated (v, u) lies outside the image has no depth (the
// reference would read out of bounds).  The count: one ballot and one integer atomic per wave.
__global__ void __launch_bounds__(256) k_rgbd(RgbdBatch B) {
    ORBGPU_LATENCY_WAVE();
    const RgbdDev& P = B.p[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool has = false;
    if (i < P.N) {
        const float x = P.keys[i].x, y = P.keys[i].y;
        float d = -1.0f;
        if (fabsf(x) < 1e9f && fabsf(y) < 1e9f) {   // (int) is defined; NaN fails
            const int u = (int)x, v = (int)y;        // C++ truncation: -0.5 -> 0
            if (u >= 0 && u < P.cols && v >= 0 && v < P.rows) {
                const uint8_t* row = P.depth + (size_t)v * P.step;
                if (P.type == kDepthU16) {
                    const uint8_t* q = row + 2 * (size_t)u;
                    d = (float)((uint32_t)q[0] | ((uint32_t)q[1] << 8));
                } else {
                    d = __uint_as_float(load_u32_any(row + 4 * (size_t)u));
                }
                if (P.convert) d = d * P.factor;
            }
        }
        has = d > 0.0f;
        P.depthOut[i] = has ? d : -1.0f;
        P.uRight[i] = has ? P.keysUn[i].x - P.mbf / d : -1.0f;
    }
    const unsigned long long m = __ballot(has);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(P.count, __popcll(m));
}

int rgbd_batch(const RgbdDev* probs, int count, hipStream_t s) {
    for (int f0 = 0; f0 < count; f0 += kRgbdPerLaunch) {
        const int n = std::min(kRgbdPerLaunch, count - f0);
        RgbdBatch B;
        std::memset(&B, 0, sizeof(B));
        int maxN = 0;
        for (int f = 0; f < n; f++) {
            B.p[f] = probs[f0 + f];
            maxN = std::max(maxN, B.p[f].N);
        }
        if (maxN > 0) hipLaunchKernelGGL(k_rgbd, dim3((maxN + 255) / 256, n), dim3(256), 0, s, B);
    }
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace orbgpu
