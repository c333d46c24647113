// capi_frame_input.cpp -- extern "C" ORBextractor_cvtColor_batch, ORBextractor_set_remap / _remap_batch and
// Frame_ComputeStereoFromRGBD[_batch] (include/orbslam_gpu.h): the cvtColor of Tracking::GrabImageStereo /
// GrabImageRGBD / GrabImageMonocular, stereo_euroc.cc's cv::remap rectification, and
// Frame::ComputeStereoFromRGBD with GrabImageRGBD's depth conversion.
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_handles.hpp"
#include "frame_input.hpp"

namespace {
size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

template <class T>
T* up(orbgpu::Matcher* m, const T* src, size_t count, hipStream_t s, int* err) {
    if (!src || count == 0) return nullptr;
    void* d = m->arena_alloc(count * sizeof(T));
    if (!d || hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess) {
        *err = ORB_E_HIP;
        return nullptr;
    }
    return (T*)d;
}

size_t depth_elem(int type) { return type == ORB_DEPTH_U16 ? 2 : 4; }
// bytes of the depth image from its first to its last pixel
size_t depth_bytes(const orb_rgbd& q) {
    if (q.cols <= 0 || q.rows <= 0) return 0;
    return q.step * (size_t)(q.rows - 1) + (size_t)q.cols * depth_elem(q.depth_type);
}

int fill_rgbd(const orb_rgbd& q, orbgpu::RgbdDev& d) {
    if (q.N < 0 || q.N > (1 << 24) || (q.N > 0 && (!q.keys || !q.keysUn || !q.depth || !q.uRight || !q.depth_out)))
        return ORB_E_INVALID;
    if (q.depth_type != ORB_DEPTH_U16 && q.depth_type != ORB_DEPTH_F32) return ORB_E_INVALID;
    if (q.cols < 0 || q.rows < 0 || q.step < (size_t)q.cols * depth_elem(q.depth_type)) return ORB_E_INVALID;
    std::memset(&d, 0, sizeof(d));
    d.N = q.N;
    d.type = q.depth_type == ORB_DEPTH_U16 ? orbgpu::kDepthU16 : orbgpu::kDepthF32;
    d.cols = q.cols;
    d.rows = q.rows;
    // GrabImageRGBD: if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F) convertTo(...)
    d.convert = std::fabs((double)(q.depthMapFactor - 1.0f)) > 1e-5 || q.depth_type != ORB_DEPTH_F32;
    d.factor = q.depthMapFactor;
    d.mbf = q.mbf;
    d.step = q.step;
    d.keys = (const orbgpu::orb_kp_dev*)q.keys;
    d.keysUn = (const orbgpu::orb_kp_dev*)q.keysUn;
    d.depth = (const uint8_t*)q.depth;
    d.uRight = q.uRight;
    d.depthOut = q.depth_out;
    return ORB_OK;
}
}  // namespace

extern "C" {

int ORBextractor_cvtColor_batch(ORBextractor_h h, const uint8_t* src, int batch, int width, int height, int channels,
                                int rgb, int step, size_t img_stride, int src_on_device, uint8_t* gray_dev,
                                int gray_step, size_t gray_stride) {
    if (!h || batch < 0 || width < 0 || height < 0 || (channels != 3 && channels != 4)) return ORB_E_INVALID;
    if (batch == 0 || width == 0 || height == 0) return ORB_OK;
    if (!src || !gray_dev || (long long)step < (long long)width * channels || gray_step < width ||
        batch > orbgpu::kCvtMaxBatch || (long long)((width + 3) / 4) * height > orbgpu::kCvtMaxQuads)
        return ORB_E_INVALID;
    // images of a batch may not overlap
    const size_t one = (size_t)step * (size_t)(height - 1) + (size_t)width * channels;
    const size_t gone = (size_t)gray_step * (size_t)(height - 1) + (size_t)width;
    if (batch > 1 && (img_stride < one || gray_stride < gone)) return ORB_E_INVALID;
    const int rc = h->ex->cvt_color(src, batch, width, height, channels, rgb != 0, step, img_stride,
                                    src_on_device != 0, gray_dev, gray_step, gray_stride);
    return rc == 0 ? ORB_OK : (rc == -2 ? ORB_E_HIP : ORB_E_INVALID);
}

int ORBextractor_set_remap(ORBextractor_h h, int slot, const float* map1, const float* map2, int dst_width,
                           int dst_height, size_t map_step, int maps_on_device) {
    if (!h || slot < 0 || slot >= ORB_REMAP_SLOTS) return ORB_E_INVALID;
    if (map1 || map2) {   // both null clears the slot
        if (!map1 || !map2 || dst_width < 1 || dst_height < 1 || dst_width > orbgpu::kRemapMaxDim ||
            dst_height > orbgpu::kRemapMaxDim || map_step < 4 * (size_t)dst_width)
            return ORB_E_INVALID;
    }
    const int rc = h->ex->set_remap(slot, map1, map2, dst_width, dst_height, map_step, maps_on_device != 0);
    return rc == 0 ? ORB_OK : (rc == -2 ? ORB_E_HIP : ORB_E_INVALID);
}

int ORBextractor_remap_batch(ORBextractor_h h, const uint8_t* src, int batch, int src_width, int src_height, int step,
                             size_t img_stride, int src_on_device, int slot0, int slot_period, uint8_t* dst_dev,
                             int dst_step, size_t dst_stride) {
    if (!h || batch < 0) return ORB_E_INVALID;
    if (batch == 0) return ORB_OK;
    if (!src || !dst_dev || batch > orbgpu::kCvtMaxBatch || src_width < 1 || src_height < 1 ||
        src_width > orbgpu::kRemapMaxDim || src_height > orbgpu::kRemapMaxDim || step < src_width)
        return ORB_E_INVALID;
    if (slot_period < 1 || slot0 < 0 || slot0 + slot_period > ORB_REMAP_SLOTS) return ORB_E_INVALID;
    // every slot an image of the batch goes through is set, and all are of one size
    int dw = 0, dh = 0;
    for (int j = 0; j < slot_period && j < batch; j++) {
        int w = 0, hh = 0;
        if (!h->ex->remap_size(slot0 + j, &w, &hh) || (j > 0 && (w != dw || hh != dh))) return ORB_E_INVALID;
        dw = w;
        dh = hh;
    }
    if (dst_step < dw) return ORB_E_INVALID;
    // images of a batch may not overlap
    const size_t one = (size_t)step * (size_t)(src_height - 1) + (size_t)src_width;
    const size_t done = (size_t)dst_step * (size_t)(dh - 1) + (size_t)dw;
    if (batch > 1 && (img_stride < one || dst_stride < done)) return ORB_E_INVALID;
    const int rc = h->ex->remap(src, batch, src_width, src_height, step, img_stride, src_on_device != 0, slot0,
                                slot_period, dst_dev, dst_step, dst_stride);
    return rc == 0 ? ORB_OK : (rc == -2 ? ORB_E_HIP : ORB_E_INVALID);
}

int Frame_ComputeStereoFromRGBD_batch(ORBmatcher_h h, int count, const orb_rgbd* R, int* ndepth) {
    if (!h || count < 0 || (count > 0 && !R)) return ORB_E_INVALID;
    if (count == 0) return ORB_OK;
    std::vector<orbgpu::RgbdDev> P((size_t)count);
    for (int f = 0; f < count; f++)
        if (int e = fill_rgbd(R[f], P[f])) return e;
    orbgpu::Matcher* m = h->m;
    const bool dev = m->device_pointers();
    hipStream_t s = m->stream();
    size_t need = al(4 * (size_t)count) + 4096;
    if (!dev)
        for (int f = 0; f < count; f++)
            need += 2 * al(sizeof(orb_kp) * (size_t)P[f].N) + 2 * al(4 * (size_t)P[f].N) + al(depth_bytes(R[f]));
    if (m->arena_reserve(need)) return ORB_E_HIP;
    // one zeroed count slot per frame: the kernel's waves add into it
    int* d_cnt = (int*)(dev ? m->count_buf(4 * (size_t)count) : m->arena_alloc(4 * (size_t)count));
    if (!d_cnt || hipMemsetAsync(d_cnt, 0, 4 * (size_t)count, s) != hipSuccess) return ORB_E_HIP;
    int err = 0;
    for (int f = 0; f < count; f++) {
        orbgpu::RgbdDev& d = P[f];
        d.count = d_cnt + f;
        if (dev || d.N == 0) continue;
        d.keys = up(m, d.keys, (size_t)d.N, s, &err);
        d.keysUn = up(m, d.keysUn, (size_t)d.N, s, &err);
        d.depth = up(m, d.depth, depth_bytes(R[f]), s, &err);
        d.uRight = (float*)m->arena_alloc(4 * (size_t)d.N);
        d.depthOut = (float*)m->arena_alloc(4 * (size_t)d.N);
        if (err || !d.uRight || !d.depthOut) return ORB_E_HIP;
    }
    if (orbgpu::rgbd_batch(P.data(), count, s)) return ORB_E_HIP;
    if (dev) {   // device mode may be deferred (ORBmatcher_set_deferred)
        if (ndepth && m->d2h_counts(ndepth, d_cnt, 4 * (size_t)count)) return ORB_E_HIP;
        return m->end_call() ? ORB_E_HIP : ORB_OK;
    }
    for (int f = 0; f < count; f++)
        if (P[f].N && (hipMemcpyAsync(R[f].uRight, P[f].uRight, 4 * (size_t)P[f].N, hipMemcpyDeviceToHost, s) !=
                           hipSuccess ||
                       hipMemcpyAsync(R[f].depth_out, P[f].depthOut, 4 * (size_t)P[f].N, hipMemcpyDeviceToHost, s) !=
                           hipSuccess))
            return ORB_E_HIP;
    if (ndepth && hipMemcpyAsync(ndepth, d_cnt, 4 * (size_t)count, hipMemcpyDeviceToHost, s) != hipSuccess)
        return ORB_E_HIP;
    return orbgpu::stream_wait(s) == hipSuccess ? ORB_OK : ORB_E_HIP;
}

int Frame_ComputeStereoFromRGBD(ORBmatcher_h h, const orb_rgbd* R, int* ndepth) {
    if (!h || !R) return ORB_E_INVALID;
    return Frame_ComputeStereoFromRGBD_batch(h, 1, R, ndepth);
}

}  // extern "C"
