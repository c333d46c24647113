// frame_input.hip -- frame input on gfx950: the RGB-D sensor path and the EuRoC stereo rectification.
//
// k_cvt_gray   Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular's cvtColor
//              (mbRGB picks RGB2GRAY or BGR2GRAY, 4 channels RGBA2GRAY / BGRA2GRAY), OpenCV 3.2's
//              8-bit path: (R*4899 + G*9617 + B*1868 + 8192) >> 14 in integers, alpha ignored.
//              "Parity unpinned" like the other OpenCV call sites.
// k_rgbd       Frame::ComputeStereoFromRGBD with the imDepth.convertTo(CV_32F, mDepthMapFactor)
//              of GrabImageRGBD folded in: the float depth image is never written, every keypoint
//              converts the one pixel it reads.
// k_remap      stereo_euroc.cc's cv::remap(im, imRect, M1, M2, INTER_LINEAR), from records that
//              k_remap_quantise makes of the two float maps once per camera (see cv::remap below).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "frame_input.hpp"

namespace orbgpu {

// 4 bytes at any address: one dword when aligned (a depth or map row pitch need not be a multiple of 4)
__device__ __forceinline__ uint32_t load_u32_any(const uint8_t* p) {
    if (((uintptr_t)p & 3) == 0) return *(const uint32_t*)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

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
int Extractor::stage_host(const uint8_t* src, size_t need, const uint8_t** dev) {
    hipStream_t s = stream_;
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
    *dev = (const uint8_t*)d_in_;
    return 0;
}

int Extractor::cvt_color(const uint8_t* src, int B, int W, int H, int channels, int rgb, int step,
                         size_t img_stride, bool src_on_device, uint8_t* gray, int gray_step, size_t gray_stride) {
    if (!src_on_device) {
        const size_t need = img_stride * (size_t)(B - 1) + (size_t)step * (size_t)(H - 1) + (size_t)W * channels;
        if (int e = stage_host(src, need, &src)) return e;
    }
    return cvt_gray_launch(src, B, W, H, channels, rgb, step, img_stride, gray, gray_step, gray_stride, stream_);
}

// ------------------------------------------------------------------ cv::remap
// stereo_euroc.cc's rectification, cv::remap(src, dst, map1, map2, INTER_LINEAR) of OpenCV 3.2
// (RemapInvoker's float-map branch, then remapBilinear<FixedPtCast<int, uchar, 15>, ..., short>);
// the five steps and why the closed-form weights are OpenCV's table are in include/orbslam_gpu.h.
// "Parity unpinned" like the other OpenCV call sites.
//
// k_remap_quantise  steps 1 and 2, once per set_remap: sx = rint(mx * 32), ix = sx >> 5,
//                   fx = sx & 31 (and y), into three uint16 planes of pitch x H records (pitch: W
//                   rounded up to a quad): ix + 1, iy + 1 and fx | fy << 5.  ix, iy in [-1, 16383]
//                   are all a source of up to 16384 can give a tap to; anything else, non-finite
//                   values included, and the padding columns are kRemapOutside: the pixel is 0
//                   for every source.  6 B per pixel instead of the maps' 8, no float work left.
// k_remap           steps 3 to 5, per frame.  One thread per 4 destination pixels of a row
//                   (k_cvt_gray's scheme): three 8-byte record loads, contiguous over the lanes,
//                   16 byte taps per image, each read only behind its own inside test (a quad whose
//                   16 tests all pass, every quad of a EuRoC map, issues them as one batch), one
//                   dword store when the destination is aligned and bytewise otherwise.  grid.y
//                   walks the images: image b uses slot lane b % period, and a thread makes `ipt`
//                   images of its lane from the record it holds in registers (ipt = 1: one image,
//                   the records of a lane are re-read from L2 by the next image's workgroups; the
//                   default, 4, measured fastest).
__global__ void __launch_bounds__(256) k_remap_quantise(const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2,
                                                        size_t map_step, int W, int pitch, long long total,
                                                        uint16_t* __restrict__ rec) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int row = (int)(t / pitch);
    const int x = (int)(t - (long long)row * pitch);
    uint32_t a = kRemapOutside, b = kRemapOutside, c = 0;
    if (x < W) {
        const size_t o = (size_t)row * map_step + 4 * (size_t)x;
        const float vx = __uint_as_float(load_u32_any(m1 + o)) * 32.0f;
        const float vy = __uint_as_float(load_u32_any(m2 + o)) * 32.0f;
        if (fabsf(vx) < 1073741824.0f && fabsf(vy) < 1073741824.0f) {   // (int) is defined; NaN fails
            const int sx = (int)rintf(vx), sy = (int)rintf(vy);         // cvRound: to nearest, ties to even
            const int ix = sx >> 5, iy = sy >> 5;
            if (ix >= -1 && ix < kRemapMaxDim && iy >= -1 && iy < kRemapMaxDim) {
                a = (uint32_t)(ix + 1);
                b = (uint32_t)(iy + 1);
                c = (uint32_t)(sx & 31) | ((uint32_t)(sy & 31) << 5);
            }
        }
    }
    rec[t] = (uint16_t)a;
    rec[total + t] = (uint16_t)b;
    rec[2 * total + t] = (uint16_t)c;
}

struct RemapArgs {
    const uint16_t* rec[ORB_REMAP_SLOTS];   // by slot lane (b % period)
    size_t plane;                           // records per plane
    int pitch, W, Q;                        // records per row; destination width, quads per row
    long long quads;
    const uint8_t* src;
    size_t img_stride;
    int sw, sh, step;
    uint8_t* dst;
    size_t dstride;
    int dstep;
    int batch, period, ipt, ny;             // ny: (lane, chunk of ipt images) pairs
};

// steps 3 to 5 for one destination pixel: a tap is read only behind its own inside test
__device__ __forceinline__ uint32_t remap_pixel(const uint8_t* __restrict__ s, int step, int sw, int sh, uint32_t a,
                                                uint32_t b, uint32_t f) {
    if (a == kRemapOutside) return 0;
    const int ix = (int)a - 1, iy = (int)b - 1;
    const uint32_t fx = f & 31u, fy = (f >> 5) & 31u;
    const bool x0 = (unsigned)ix < (unsigned)sw, x1 = (unsigned)(ix + 1) < (unsigned)sw;
    uint32_t s00 = 0, s01 = 0, s10 = 0, s11 = 0;
    if ((unsigned)iy < (unsigned)sh) {
        const uint8_t* r = s + (size_t)iy * (size_t)step;
        if (x0) s00 = r[ix];
        if (x1) s01 = r[ix + 1];
    }
    if ((unsigned)(iy + 1) < (unsigned)sh) {
        const uint8_t* r = s + (size_t)(iy + 1) * (size_t)step;
        if (x0) s10 = r[ix];
        if (x1) s11 = r[ix + 1];
    }
    const uint32_t gx = 32u - fx, gy = 32u - fy;
    return (s00 * (32u * gx * gy) + s01 * (32u * fx * gy) + s10 * (32u * gx * fy) + s11 * (32u * fx * fy) + 16384u) >>
           15;
}

__global__ void __launch_bounds__(256) k_remap(RemapArgs A) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= A.quads) return;
    const int row = (int)(t / A.Q);
    const int x0 = 4 * (int)(t - (long long)row * A.Q);
    const int n = min(4, A.W - x0);
    for (int y = blockIdx.y; y < A.ny; y += gridDim.y) {
        const int lane = y % A.period, chunk = y / A.period;
        const uint16_t* r = A.rec[lane] + (size_t)row * (size_t)A.pitch + (size_t)x0;
        const uint2 ra = *(const uint2*)r, rb = *(const uint2*)(r + A.plane), rf = *(const uint2*)(r + 2 * A.plane);
        const uint32_t a[4] = {ra.x & 0xFFFFu, ra.x >> 16, ra.y & 0xFFFFu, ra.y >> 16};
        const uint32_t b[4] = {rb.x & 0xFFFFu, rb.x >> 16, rb.y & 0xFFFFu, rb.y >> 16};
        const uint32_t f[4] = {rf.x & 0xFFFFu, rf.x >> 16, rf.y & 0xFFFFu, rf.y >> 16};
        // every tap of the quad inside the source: ix = a - 1 in [0, sw - 2] and iy = b - 1 in
        // [0, sh - 2] for all four pixels (0, kRemapOutside and the padding past W fail the compare)
        bool inner = true;
#pragma unroll
        for (int p = 0; p < 4; p++)
            inner = inner && (a[p] - 1u) < (uint32_t)(A.sw - 1) && (b[p] - 1u) < (uint32_t)(A.sh - 1);
        for (int k = 0; k < A.ipt; k++) {
            const long long img = lane + (long long)A.period * ((long long)chunk * A.ipt + k);
            if (img >= A.batch) break;
            const uint8_t* s = A.src + (size_t)img * A.img_stride;
            uint8_t* d = A.dst + (size_t)img * A.dstride + (size_t)row * (size_t)A.dstep + (size_t)x0;
            uint32_t g[4];
            if (inner) {   // all 16 tests passed: the taps as one batch of loads, no branch between them
                uint32_t v[4][4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const uint8_t* q = s + (size_t)(b[p] - 1) * (size_t)A.step + (size_t)(a[p] - 1);
                    v[p][0] = q[0];
                    v[p][1] = q[1];
                    v[p][2] = q[A.step];
                    v[p][3] = q[A.step + 1];
                }
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const uint32_t fx = f[p] & 31u, fy = (f[p] >> 5) & 31u, gx = 32u - fx, gy = 32u - fy;
                    g[p] = (v[p][0] * (32u * gx * gy) + v[p][1] * (32u * fx * gy) + v[p][2] * (32u * gx * fy) +
                            v[p][3] * (32u * fx * fy) + 16384u) >> 15;
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) g[p] = remap_pixel(s, A.step, A.sw, A.sh, a[p], b[p], f[p]);
            }
            if (n == 4 && ((uintptr_t)d & 3) == 0) {
                *(uint32_t*)d = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (p < n) d[p] = (uint8_t)g[p];
            }
        }
    }
}

int Extractor::retire(void* p, bool host) {
    Retired r{p, host, nullptr};
    if (hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess ||
        hipEventRecord(r.ev, stream_) != hipSuccess) {
        // no event to wait for: wait for the stream itself (set_remap is not the per-frame path)
        if (r.ev) (void)hipEventDestroy(r.ev);
        (void)hipStreamSynchronize(stream_);
        if (host) (void)hipHostFree(p); else (void)hipFree(p);
        return -2;
    }
    retired_.push_back(r);
    return 0;
}

void Extractor::sweep_retired(bool wait) {
    size_t keep = 0;
    for (size_t i = 0; i < retired_.size(); i++) {
        Retired& r = retired_[i];
        if (wait) (void)hipEventSynchronize(r.ev);
        if (wait || hipEventQuery(r.ev) == hipSuccess) {
            (void)hipEventDestroy(r.ev);
            if (r.host) (void)hipHostFree(r.p); else (void)hipFree(r.p);
        } else {
            retired_[keep++] = r;
        }
    }
    retired_.resize(keep);
}

void Extractor::release_remap() {
    sweep_retired(true);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (RemapSlot& sl : remap_) {
        if (sl.rec) (void)hipFree(sl.rec);
        sl = RemapSlot();
    }
}

bool Extractor::remap_size(int slot, int* w, int* h) const {
    if (slot < 0 || slot >= ORB_REMAP_SLOTS || !remap_[slot].rec) return false;
    *w = remap_[slot].w;
    *h = remap_[slot].h;
    return true;
}

// The old records may still be read by a queued k_remap: they are retired behind an event on the
// stream, and freed by a later set_remap (or the destructor) once that event is done.  Host maps are
// packed into a pinned block (also retired) and copied on the stream, so nothing here waits.
int Extractor::set_remap(int slot, const float* map1, const float* map2, int W, int H, size_t map_step,
                         bool on_device) {
    hipStream_t s = stream_;
    sweep_retired(false);
    RemapSlot& sl = remap_[slot];
    if (sl.rec) {
        void* old = sl.rec;
        sl = RemapSlot();
        if (int e = retire(old, false)) return e;
    }
    if (!map1 && !map2) return 0;
    const int pitch = 4 * ((W + 3) / 4);
    const long long total = (long long)pitch * H;
    uint16_t* rec = nullptr;
    ORB_HIP_CHECK(hipMalloc(&rec, 3 * sizeof(uint16_t) * (size_t)total));
    const uint8_t *m1 = (const uint8_t*)map1, *m2 = (const uint8_t*)map2;
    if (!on_device) {
        const size_t row = 4 * (size_t)W, one = row * (size_t)H;
        uint8_t* hp = nullptr;
        uint8_t* dp = nullptr;
        if (hipHostMalloc(&hp, 2 * one) != hipSuccess || hipMalloc(&dp, 2 * one) != hipSuccess) {
            if (hp) (void)hipHostFree(hp);
            (void)hipFree(rec);
            return -2;
        }
        for (int r = 0; r < H; r++) {
            std::memcpy(hp + row * r, m1 + map_step * r, row);
            std::memcpy(hp + one + row * r, m2 + map_step * r, row);
        }
        const hipError_t ce = hipMemcpyAsync(dp, hp, 2 * one, hipMemcpyHostToDevice, s);
        m1 = dp;
        m2 = dp + one;
        map_step = row;
        hipLaunchKernelGGL(k_remap_quantise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, m1, m2, map_step,
                           W, pitch, total, rec);
        const hipError_t ke = hipGetLastError();
        const int r1 = retire(hp, true), r2 = retire(dp, false);
        if (ce != hipSuccess || ke != hipSuccess || r1 || r2) {
            (void)retire(rec, false);
            return -2;
        }
    } else {
        hipLaunchKernelGGL(k_remap_quantise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, m1, m2, map_step,
                           W, pitch, total, rec);
        if (hipGetLastError() != hipSuccess) {
            (void)retire(rec, false);
            return -2;
        }
    }
    sl.rec = rec;
    sl.w = W;
    sl.h = H;
    sl.pitch = pitch;
    return 0;
}

int Extractor::remap(const uint8_t* src, int B, int sw, int sh, int step, size_t img_stride, bool src_on_device,
                     int slot0, int period, uint8_t* dst, int dst_step, size_t dst_stride) {
    if (B <= 0) return 0;
    const RemapSlot& first = remap_[slot0];
    if (!src_on_device) {
        const size_t need = img_stride * (size_t)(B - 1) + (size_t)step * (size_t)(sh - 1) + (size_t)sw;
        if (int e = stage_host(src, need, &src)) return e;
    }
    RemapArgs A;
    std::memset(&A, 0, sizeof(A));
    period = std::min(period, B);   // lanes past the batch have no image
    for (int j = 0; j < period; j++) A.rec[j] = remap_[slot0 + j].rec;
    A.pitch = first.pitch;
    A.plane = (size_t)first.pitch * (size_t)first.h;
    A.W = first.w;
    A.Q = first.pitch / 4;
    A.quads = (long long)A.Q * first.h;
    A.src = src;
    A.img_stride = img_stride;
    A.sw = sw;
    A.sh = sh;
    A.step = step;
    A.dst = dst;
    A.dstride = dst_stride;
    A.dstep = dst_step;
    A.batch = B;
    A.period = period;
    int ipt = kRemapImagesPerThread;
    if (const char* e = std::getenv("ORBGPU_REMAP_IPT")) ipt = std::atoi(e);   // measurement (tools/remap_timing.py)
    const int per_lane = (B + period - 1) / period;
    A.ipt = std::max(1, std::min(ipt, per_lane));
    A.ny = period * ((per_lane + A.ipt - 1) / A.ipt);
    const dim3 grid((unsigned)((A.quads + 255) / 256), (unsigned)std::min(A.ny, 65535));
    hipLaunchKernelGGL(k_remap, grid, dim3(256), 0, stream_, A);
    ORB_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------ ComputeStereoFromRGBD
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
