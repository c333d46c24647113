/*
 * orbslam_gpu.h -- C ABI of the MI355X-native ORB-SLAM2 per-frame hot path.
 *
 * Drop-in boundary for junejunejune/c_orb_slam (ORB-SLAM2, C++11).  The
 * reference exposes these operations as C++ class methods taking cv::Mat /
 * std::vector; each entry point below replaces one of them with plain
 * pointers + sizes.  The C++ adapter in
 * c_orb_slam_amd/adapter/ re-exposes the reference class signatures on top
 * of this header; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - every call returns int status: ORB_OK (0) or a negative ORB_E_*;
 *   - the caller owns all host buffers (pointer + capacity; counts are
 *     written to *n_out; ORB_E_CAPACITY if a buffer is too small);
 *   - each handle owns its device workspace and one HIP stream; handles are
 *     not shared between threads (the reference calls the extractor from two
 *     threads per stereo frame, Frame.cc:78-81: create one handle per thread);
 *   - there is no CPU fallback: without a usable gfx950 device, create()
 *     returns ORB_E_NODEVICE.
 */
#ifndef ORBSLAM_GPU_H
#define ORBSLAM_GPU_H
#include <stdbool.h>
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORB_OK 0
#define ORB_E_INVALID -1
#define ORB_E_HIP -2
#define ORB_E_CAPACITY -3
#define ORB_E_NODEVICE -4

/* cv::KeyPoint memory layout (28 B): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct orb_kp {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orb_kp;

/* Library info: 1 if a HIP device is usable, else 0 (never aborts). */
int orbgpu_device_available(void);
const char* orbgpu_version(void);
/* ABI revision of this header.  A caller compiled against revision R checks
 * orbgpu_abi_version() == R at start-up: an entry point whose signature changed bumps it.
 *   1: round 1-3 ABI
 *   2: ORBmatcher_SearchLocalPoints_batch takes the ORBmatcher(nnratio) float before the
 *      outputs (a revision-1 binary would pass its pointers with nnratio undefined) */
#define ORBGPU_ABI_VERSION 2
int orbgpu_abi_version(void);

/* ======================================================================
 * ORBextractor  (reference include/ORBextractor.h:51-113, src/ORBextractor.cc)
 * ====================================================================== */
typedef struct ORBextractor_t* ORBextractor_h;

/* ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels,
 *                            int iniThFAST, int minThFAST)   ORBextractor.cc:410-470
 * max_width/max_height size the device pyramid (images up to that size). */
int ORBextractor_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                        int minThFAST, int max_width, int max_height, int max_batch,
                        ORBextractor_h* out);
int ORBextractor_destroy(ORBextractor_h h);

/* ORBextractor::operator()(image, mask(ignored), keypoints, descriptors)
 *                                                          ORBextractor.cc:1043-1105
 * img: u8 grey, row stride `step`.  kps: capacity entries; desc: capacity x 32.
 * Empty image (w or h == 0) returns ORB_OK with *n_out = 0 (1046-1047). */
int ORBextractor_extract(ORBextractor_h h, const uint8_t* img, int width, int height, int step,
                         orb_kp* kps, uint8_t* desc, int capacity, int* n_out);

/* Batched form: `batch` images of equal size; image b at imgs + b*img_stride.
 * imgs_on_device != 0: imgs is a device pointer (HBM-resident input).
 * Outputs for image b at kps + b*cap_per_image, desc + b*cap_per_image*32;
 * outputs_on_device != 0: kps/desc are device pointers.  n_out[b] host. */
int ORBextractor_extract_batch(ORBextractor_h h, const uint8_t* imgs, int batch, int width,
                               int height, int step, size_t img_stride, int imgs_on_device,
                               orb_kp* kps, uint8_t* desc, int cap_per_image,
                               int outputs_on_device, int* n_out);

/* Host images at separate addresses: Frame(imLeft, imRight)'s two cv::Mat (Frame.cc:78-81 runs
 * the left and right extractors on two threads; here both are one call on one stream).  Image b
 * at imgs[b] (host, row stride `step`); the images are staged in one pinned block and copied to
 * HBM with one H2D copy.  Outputs as ORBextractor_extract_batch (image b at kps + b*cap). */
int ORBextractor_extract_images(ORBextractor_h h, const uint8_t* const* imgs, int batch, int width,
                                int height, int step, orb_kp* kps, uint8_t* desc, int cap_per_image,
                                int outputs_on_device, int* n_out);

/* cv::cvtColor(im, im, CV_RGB2GRAY | CV_BGR2GRAY | CV_RGBA2GRAY | CV_BGRA2GRAY) as
 * Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular apply it to a 3- or 4-channel
 * image (mbRGB picks the order) before the Frame is built.  OpenCV 3.2's 8-bit path: per pixel
 * (R*4899 + G*9617 + B*1868 + 8192) >> 14 in integers, alpha ignored; "parity unpinned" at this
 * OpenCV call site.  rgb != 0: the first byte of a pixel is R, otherwise B.
 * `batch` images of equal size, image b at src + b*img_stride (rows `step` >= width*channels
 * bytes apart; src_on_device != 0: a device pointer, otherwise host memory that is staged through
 * the extractor's pinned block as ORBextractor_extract_images stages its images).  The result is
 * always a device image: grey image b at gray_dev + b*gray_stride, rows gray_step >= width bytes
 * apart; no alignment is required of either side, and the images of a batch may not overlap
 * (batch <= 65535).  The call is enqueued on ORBextractor_stream(h)
 * and does not wait: a following ORBextractor_extract_batch(h, gray_dev, ..., imgs_on_device = 1,
 * ...) on the same handle sees the grey images.  channels = 3 or 4 (the reference makes no call
 * for a 1-channel image: ORB_E_INVALID); width, height or batch 0: ORB_OK, nothing is done. */
int ORBextractor_cvtColor_batch(ORBextractor_h h, const uint8_t* src, int batch, int width, int height,
                                int channels, int rgb, int step, size_t img_stride, int src_on_device,
                                uint8_t* gray_dev, int gray_step, size_t gray_stride);

/* Stereo rectification of Examples/Stereo/stereo_euroc.cc: after
 *   cv::initUndistortRectifyMap(K_l, D_l, R_l, P_l(3x3), size, CV_32F, M1l, M2l)      (once)
 * every frame goes through cv::remap(imLeft, imLeftRect, M1l, M2l, cv::INTER_LINEAR) (and the right
 * image through M1r, M2r) before TrackStereo.  The maps are taken as the driver computed them:
 * initUndistortRectifyMap itself stays with OpenCV (once per camera, in double, its bits depend on
 * the OpenCV build).
 *
 * The specification is OpenCV 3.2 imgwarp.cpp, RemapInvoker's float-map branch and then
 * remapBilinear<FixedPtCast<int, uchar, 15>, ..., short>.  For a destination pixel with map values
 * mx, my (float32):
 *   1. sx = cvRound(mx * 32), sy = cvRound(my * 32): a float32 multiply (exact, 32 is a power of
 *      two), rounded to nearest, ties to even (rintf; _mm_cvtps_epi32 in the SIMD path);
 *   2. ix = sx >> 5, iy = sy >> 5 (arithmetic: a floor), fx = sx & 31, fy = sy & 31.  OpenCV
 *      saturates ix, iy to short: with sizes up to 16384 a saturated value is outside the image
 *      either way.  A non-finite map value, or one with |m * 32| >= 2^30, counts as far outside and
 *      the pixel is 0 (a stated simplification of an int conversion that x86 leaves at INT_MIN; the
 *      byte is the same);
 *   3. the taps S(iy, ix), S(iy, ix+1), S(iy+1, ix), S(iy+1, ix+1): a tap inside
 *      [0, src_width) x [0, src_height) reads the source, a tap outside is 0 and is never addressed
 *      (OpenCV's inlier, fully-outside and BORDER_CONSTANT straddling branches in one rule);
 *   4. w00 = 32(32-fx)(32-fy), w01 = 32 fx (32-fy), w10 = 32(32-fx) fy, w11 = 32 fx fy, in integers;
 *      they sum to 32768;
 *   5. dst = (S00 w00 + S01 w01 + S10 w10 + S11 w11 + 16384) >> 15, at most 255.
 * The closed form of step 4 is OpenCV's table: initInterTab2D stores
 * saturate_cast<short>(vy * vx * 32768) with vx in {1 - fx/32, fx/32} and vy likewise, products of
 * 5-bit ratios that are exact in float and after scaling.  The one value a short cannot hold is
 * 32768 at fx = fy = 0; there OpenCV stores 32767 and its sum fix-up adds the missing 1 to another
 * entry of the 2 x 2 block, and (S00*32767 + S*1 + 16384) >> 15 == S00 for all bytes S00, S, so the
 * output byte is the same.  "Parity unpinned" at this OpenCV call site, as cvtColor:
 * the restatement is tests/remap_ref.py.  One channel, INTER_LINEAR, BORDER_CONSTANT with value 0:
 * the only form the reference calls. */
#define ORB_REMAP_SLOTS 4

/* The two CV_32FC1 maps of cv::initUndistortRectifyMap(..., CV_32F, map1, map2) as the driver
 * computed them (stereo_euroc.cc: M1l/M2l, M1r/M2r), kept on the handle in `slot`
 * (0 .. ORB_REMAP_SLOTS-1).  dst_width x dst_height (1 .. 16384 each) is the size of the maps and of
 * every image remapped through the slot; rows of both maps are map_step bytes apart
 * (>= 4*dst_width); no alignment is required.  maps_on_device != 0: device pointers, read by a
 * kernel enqueued on ORBextractor_stream(h) (they must stay valid until the stream has passed it;
 * host maps are copied before the call returns).  The maps are quantised once, here (steps 1 and
 * 2), into 6 bytes per pixel.  Replaces what the slot held: a remap through the slot that is
 * still queued sees the old maps.  map1 == NULL && map2 == NULL clears the slot. */
int ORBextractor_set_remap(ORBextractor_h h, int slot, const float* map1, const float* map2,
                           int dst_width, int dst_height, size_t map_step, int maps_on_device);

/* cv::remap(src, dst, map1, map2, cv::INTER_LINEAR) with its defaults (BORDER_CONSTANT, value 0)
 * for `batch` 8-bit 1-channel images of src_width x src_height (1 .. 16384 each), image b at
 * src + b*img_stride, rows `step` >= src_width bytes apart, host (staged like
 * ORBextractor_cvtColor_batch's source) or device.  Image b goes through slot
 * slot0 + b % slot_period, so slot_period 1 means one camera and slot_period 2 means left / right
 * interleaved.  Every slot used must be set and of equal size.  The result is always a device
 * image of the slot's size: image b at dst_dev + b*dst_stride, rows dst_step >= dst_width bytes
 * apart.  No alignment is required of any pointer or pitch; the images of a batch may not overlap
 * (img_stride and dst_stride are checked when batch > 1); batch <= 65535, and a batch of 0 returns
 * ORB_OK and does nothing.  Null pointers, an unset slot, slots of unequal size, slot_period < 1,
 * slot0 < 0 or slot0 + slot_period > ORB_REMAP_SLOTS and a pitch below a row's bytes return
 * ORB_E_INVALID before any device work.  Enqueued on ORBextractor_stream(h), does not wait: a
 * following ORBextractor_extract_batch(h, dst_dev, ..., imgs_on_device = 1, ...) on the same
 * handle sees the rectified images. */
int ORBextractor_remap_batch(ORBextractor_h h, const uint8_t* src, int batch, int src_width,
                             int src_height, int step, size_t img_stride, int src_on_device,
                             int slot0, int slot_period, uint8_t* dst_dev, int dst_step,
                             size_t dst_stride);

/* mvImagePyramid[level] (ORBextractor.h:85) of image `index` of the last call,
 * copied to host WITH its 19-px REFLECT_101 border (Frame.cc:573-580 reads it).
 * dst must hold (w+38)*(h+38) bytes at stride dst_step; *w,*h = unpadded dims. */
int ORBextractor_get_level(ORBextractor_h h, int index, int level, uint8_t* dst, int dst_step,
                           int* w, int* h_);
/* Diagnostic: the GaussianBlur(7x7, 2) working image of `level` (ORBextractor.cc:1085-1086,
 * no border) of image `index` of the last call; dst holds w*h bytes at dst_step. */
int ORBextractor_get_blurred_level(ORBextractor_h h, int index, int level, uint8_t* dst,
                                   int dst_step, int* w, int* h_);
/* GetLevels/GetScaleFactor/GetScaleFactors/GetInverseScaleFactors/
 * GetScaleSigmaSquares/GetInverseScaleSigmaSquares   ORBextractor.h:63-85 */
int ORBextractor_get_levels(ORBextractor_h h, int* nlevels, float* scaleFactor);
int ORBextractor_get_scale_tables(ORBextractor_h h, float* scale, float* invScale,
                                  float* sigma2, float* invSigma2, int* nFeaturesPerLevel);
/* HIP stream (hipStream_t) the extractor launches on; for event timing. */
void* ORBextractor_stream(ORBextractor_h h);
/* Per-stage device time of the last call (ms), from HIP events:
 * [0]=pyramid [1]=blur [2]=FAST cells [3]=compaction [4]=octree(host) [5]=orientation+rBRIEF */
int ORBextractor_last_timings(ORBextractor_h h, float* ms6);
/* FAST corners kept by the last call, summed over its images (after the per-cell NMS and cell
 * caps of ORBextractor.cc:776-829, before DistributeOctTree): the k_fast_cells output that the
 * bench's algorithmic-bytes figure counts. */
int ORBextractor_last_corner_count(ORBextractor_h h, long long* total);
/* Scheduling (no reference counterpart): keep one CU in every `one_in_n` of each XCD out of
 * this extractor's launches (its stream is recreated with a CU mask), so the tracking lane's
 * one-workgroup-per-frame kernels (matcher greedy replay, PoseOptimization) find free wave
 * slots while a batch is being extracted.  one_in_n = 0 restores the full device.  Call
 * between extractions; ORBextractor_stream() changes. */
int ORBextractor_reserve_cus(ORBextractor_h h, int one_in_n);
/* Scheduling (no reference counterpart): h launches on `with`'s stream from now on, so the
 * extractions of two extractors queue back to back on the device in call order (a pipeline
 * that enqueues batch k+1 while batch k runs leaves no gap between them).  `with` keeps owning
 * the stream and must outlive h; ORBextractor_reserve_cus is refused on both afterwards. */
int ORBextractor_share_stream(ORBextractor_h h, ORBextractor_h with);

/* ======================================================================
 * ORBmatcher  (reference include/ORBmatcher.h:41-103, src/ORBmatcher.cc)
 * ====================================================================== */
typedef struct ORBmatcher_t* ORBmatcher_h;

/* ORBmatcher::ORBmatcher(float nnratio=0.6, bool checkOri=true)  ORBmatcher.cc:41-43 */
int ORBmatcher_create(float nnratio, int checkOri, ORBmatcher_h* out);
int ORBmatcher_destroy(ORBmatcher_h h);
/* Pointer space of every array argument below (and inside orb_frame /
 * orb_mappoints): 0 = host memory (default, copied per call), 1 = device
 * (HBM-resident, e.g. ORBextractor_extract_batch outputs); counts stay host. */
int ORBmatcher_set_device_pointers(ORBmatcher_h h, int on);
void* ORBmatcher_stream(ORBmatcher_h h);

/* Measurement (no reference counterpart; bench roofline): with timing on, every search,
 * stereo and CSR call on this matcher records HIP events around its kernels on
 * ORBmatcher_stream() and counts its work on the device.  ORBmatcher_last_timings waits for
 * the stream and returns the last call's kernel times (ms, -1 = not run):
 *   ms8[0..6]: k_build_grid, k_candidates, k_select, k_stereo_rows, k_stereo_match,
 *              k_stereo_filter, k_csr_hamming;
 * and work counts:
 *   counts8[0..5]: SearchByProjection (query, candidate) pairs scored, queries with a window,
 *                  ComputeStereoMatches (left, right) pairs scored, left keypoints searched,
 *                  SearchCandidates pairs, SearchCandidates queries;
 *   counts8[7]: ComputeStereoMatches left keypoints whose 11x11 SAD windows were read. */
int ORBmatcher_enable_timing(ORBmatcher_h h, int on);
int ORBmatcher_last_timings(ORBmatcher_h h, float* ms8, long long* counts8);
/* Test-only, read-only: which launches the last guided search of `h` chose
 * (ORBmatcher_SearchByProjection_LastFrame[_batch], ORBmatcher_SearchByProjection_MapPoints,
 * ORBmatcher_SearchLocalPoints_batch).  out[0]: 1 the candidate search staged the frame in LDS,
 * 0 it walked the grid in device memory (a frame of the batch above 1536 keypoints, or
 * ORBGPU_CAND_LOCAL_STAGE=0); out[1]: threads per candidate workgroup (1024, or 256 unstaged or
 * with ORBGPU_CAND_NT=256); out[2]: threads per selection workgroup (512 last-frame, 1024 local,
 * 512 local with ORBGPU_SELECT_LOCAL_NT=512); out[1] = out[2] = 0 when no problem had a query
 * (nothing but the grid build ran); out[3]: the largest frame keypoint count of the batch;
 * out[4]: the largest query count; out[5]: the number of problems.  Host state only.
 * ORB_E_INVALID before the first search that reached its launches. */
int ORBmatcher_last_search_plan(ORBmatcher_h h, int out[6]);
/* Deferred completion (no reference counterpart; the reference's calls are synchronous).
 * With deferred on (device-pointer matchers only), the device-resident batch calls
 * ORBmatcher_ComputeStereoMatches_batch, MapPoint_CreateStereo_batch_device,
 * ORBmatcher_SearchByProjection_LastFrame_batch, Tracking_PrepareLocalSearch_batch_device,
 * ORBmatcher_SearchLocalPoints_batch and Optimizer_PoseOptimization_frames_device_deferred
 * return as soon as their work is queued on ORBmatcher_stream(h); their per-problem counts
 * (nmatches, nvisible, ninliers) are written when ORBmatcher_finish(h) returns.  A chain of
 * TrackWithMotionModel + TrackLocalMap calls then runs without a host round trip between
 * the calls.  Turning deferred off finishes a pending chain. */
int ORBmatcher_set_deferred(ORBmatcher_h h, int on);
int ORBmatcher_finish(ORBmatcher_h h);
/* Overlapping chains: close the calls queued so far into an epoch (returns at once), queue the
 * next step's calls, and finish the older epoch later.  chain_wait blocks until an epoch's
 * device work is done (no counts written; callable from another host thread, e.g. before
 * reusing that epoch's input buffers); chain_finish(e) waits for every epoch <= e and writes
 * their counts. */
int ORBmatcher_chain_close(ORBmatcher_h h, long long* epoch);
int ORBmatcher_chain_wait(ORBmatcher_h h, long long epoch);
int ORBmatcher_chain_finish(ORBmatcher_h h, long long epoch);

/* static int ORBmatcher::DescriptorDistance(a, b)   ORBmatcher.cc:1647-1663 (host) */
int ORBmatcher_DescriptorDistance(const uint8_t* a, const uint8_t* b);

/* Frame view used for guided search (Frame.h fields the matcher reads).
 * Grid: Frame::mGrid (64 x 48, Frame.h:37-38) is rebuilt on device from
 * kpsUn (AssignFeaturesToGrid, Frame.cc:230-245). */
typedef struct orb_frame {
    int N;
    const orb_kp* keysUn;        /* mvKeysUn (N) */
    const uint8_t* desc;         /* mDescriptors (N x 32) */
    const float* uRight;         /* mvuRight (N) or NULL (monocular) */
    float minX, maxX, minY, maxY;/* mnMinX.. (Frame.cc:442-470) */
    float gridWInv, gridHInv;    /* mfGridElementWidthInv/HeightInv */
    const float* scaleFactors;   /* mvScaleFactors */
    int nlevels;
    float fx, fy, cx, cy, bf, b; /* intrinsics, mbf, mb */
    const float* Tcw;            /* 4x4 row-major float (mTcw) */
} orb_frame;

/* Map point table shared by the search calls (MapPoint fields read by the matcher). */
typedef struct orb_mappoints {
    int n;
    const float* pos;            /* GetWorldPos (n x 3) */
    const uint8_t* desc;         /* GetDescriptor (n x 32) */
    const int* observations;     /* Observations() (n) */
} orb_mappoints;

/* int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool bMono)
 *                                                          ORBmatcher.cc:1328-1470
 * last_mp[i]: map point index of LastFrame.mvpMapPoints[i] (-1 = NULL);
 * last_outlier[i]: LastFrame.mvbOutlier; last_keys: LastFrame.mvKeys (octave),
 * last_keysUn: LastFrame.mvKeysUn (angle).
 * cur_mp (in/out, N of current): CurrentFrame.mvpMapPoints as indices (-1 = NULL).
 * *nmatches = return value of the reference (0 when the last frame has no keypoint).
 * Both frames hold at most 4096 keypoints: ORB_E_INVALID above, with nothing written. */
int ORBmatcher_SearchByProjection_LastFrame(ORBmatcher_h h, const orb_frame* cur, int32_t* cur_mp,
                                            const orb_frame* last, const orb_kp* last_keys,
                                            const int32_t* last_mp, const uint8_t* last_outlier,
                                            const orb_mappoints* mps, float th, int bMono,
                                            int* nmatches);

/* Batched form of the above over `npairs` independent (cur, last) pairs in ONE launch. */
int ORBmatcher_SearchByProjection_LastFrame_batch(ORBmatcher_h h, int npairs, const orb_frame* cur,
                                                  int32_t* const* cur_mp, const orb_frame* last,
                                                  const orb_kp* const* last_keys,
                                                  const int32_t* const* last_mp,
                                                  const uint8_t* const* last_outlier,
                                                  const orb_mappoints* mps, float th, int bMono,
                                                  int* nmatches);

/* int SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, float th)
 *                                                          ORBmatcher.cc:45-129
 * Per map point j (order = vpMapPoints order): track_in_view (mbTrackInView),
 * proj_x/proj_xr/proj_y (mTrackProjX/XR/Y), level (mnTrackScaleLevel),
 * view_cos (mTrackViewCos), mp_index (index into mps, written to cur_mp). */
int ORBmatcher_SearchByProjection_MapPoints(ORBmatcher_h h, const orb_frame* F, int32_t* cur_mp,
                                            int n, const uint8_t* track_in_view,
                                            const float* proj_x, const float* proj_xr,
                                            const float* proj_y, const int32_t* level,
                                            const float* view_cos, const int32_t* mp_index,
                                            const orb_mappoints* mps, float th, int* nmatches);

/* Tracking::mvpLocalMapPoints with the MapPoint fields isInFrustum and SearchByProjection read. */
typedef struct orb_localmap {
    int n;
    const float* pos;            /* GetWorldPos (n x 3) */
    const uint8_t* desc;         /* GetDescriptor (n x 32) */
    const int* observations;     /* Observations() (n) */
    const float* max_dist;       /* mfMaxDistance (n) */
    const float* min_dist;       /* mfMinDistance (n) */
    const float* normal;         /* GetNormal() (n x 3) */
    const uint8_t* skip;         /* mnLastFrameSeen == CurrentFrame.mnId, or isBad() (n) */
} orb_localmap;

/* bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit)      Frame.cc:269-325
 * For every point of maps[p] not skipped: the visibility test against frame F[p] (Tcw, bounds,
 * intrinsics, mbf, nlevels) and the MapPoint tracking fields it fills: in_view (mbTrackInView),
 * proj_x / proj_xr / proj_y (mTrackProjX / XR / Y), level (mnTrackScaleLevel, PredictScale),
 * view_cos (mTrackViewCos); outputs of points not in view are left untouched except in_view = 0.
 * nvisible[p] = points in view.  Device pointers only; desc / observations of maps unused. */
int Frame_isInFrustum_batch(ORBmatcher_h h, int count, const orb_frame* F, const orb_localmap* maps,
                            float viewingCosLimit, float logScaleFactor, uint8_t* const* in_view,
                            float* const* proj_x, float* const* proj_xr, float* const* proj_y,
                            int32_t* const* level, float* const* view_cos, int* nvisible);

/* void Tracking::SearchLocalPoints()                          Tracking.cc:1143-1193
 * For every local map point not skipped: Frame::isInFrustum(pMP, 0.5) (Frame.cc:269-325,
 * MapPoint::PredictScale MapPoint.cc:402-417), then SearchByProjection(F, mvpLocalMapPoints,
 * th) with ratio `nnratio` (the reference constructs ORBmatcher matcher(0.8) for this search,
 * Tracking.cc:1184; ORBmatcher.cc:45-129): pass 0.8 to follow it on any matcher, or <= 0 to
 * use the matcher's own nnratio (so one deferred chain serves every search of a step).
 * cur_mp[p] (in/out, F[p].N): mCurrentFrame.mvpMapPoints as rows of maps[p] (-1 = NULL);
 * the caller clears the outliers of the first PoseOptimization and marks the matched and
 * discarded points in `skip` first (Tracking.cc:893-913, 1146-1161).  logScaleFactor =
 * Frame::mfLogScaleFactor.  nmatches[p] = SearchByProjection's return value, nvisible[p] =
 * nToMatch (points IncreaseVisible() counts).  Device pointers only (ORBmatcher_set_device_
 * pointers(h, 1)); one launch set for all `count` frames. */
int ORBmatcher_SearchLocalPoints_batch(ORBmatcher_h h, int count, const orb_frame* F, int32_t* const* cur_mp,
                                       const orb_localmap* maps, float logScaleFactor, float th,
                                       float nnratio, int* nmatches, int* nvisible);

/* void Frame::ComputeStereoMatches()                            Frame.cc:466-640
 * Rectified stereo matching of the left keypoints of image `index` (0 only for the single
 * form; image p of the batch form) of the last ORBextractor_extract[_batch] call of `left`
 * and `right`: mvImagePyramid (with border) is read from those extractors, the scale
 * tables from `left`.  keysL/descL: mvKeys/mDescriptors (NL), keysR/descR: mvKeysRight /
 * mDescriptorsRight (NR).  mbf, mb: Frame::mbf, mb.  Outputs mvuRight / mvDepth (NL
 * floats, -1 = no stereo) and *nmatches = the stereo matches kept after the median filter.
 * Pointer space per ORBmatcher_set_device_pointers.  NL <= 4096. */
int ORBmatcher_ComputeStereoMatches(ORBmatcher_h h, ORBextractor_h left, ORBextractor_h right, int index,
                                    int NL, const orb_kp* keysL, const uint8_t* descL, int NR,
                                    const orb_kp* keysR, const uint8_t* descR, float mbf, float mb,
                                    float* uRight, float* depth, int* nmatches);
/* `npairs` stereo pairs (images 0..npairs-1 of the last batch calls) in one launch. */
int ORBmatcher_ComputeStereoMatches_batch(ORBmatcher_h h, ORBextractor_h left, ORBextractor_h right,
                                          int npairs, const int* NL, const orb_kp* const* keysL,
                                          const uint8_t* const* descL, const int* NR,
                                          const orb_kp* const* keysR, const uint8_t* const* descR,
                                          float mbf, float mb, float* const* uRight,
                                          float* const* depth, int* nmatches);
/* The same with pair p = (image first_left + p of `left`'s last batch, image first_right + p of
 * `right`'s): both images of every pair may come from ONE extractor's batch call over
 * [lefts..., rights...] (left == right, first_right = npairs), i.e. Frame(imLeft, imRight)'s two
 * extractions (Frame.cc:78-81) as one batch launch set. */
int ORBmatcher_ComputeStereoMatches_batch_at(ORBmatcher_h h, ORBextractor_h left, int first_left,
                                             ORBextractor_h right, int first_right, int npairs,
                                             const int* NL, const orb_kp* const* keysL,
                                             const uint8_t* const* descL, const int* NR,
                                             const orb_kp* const* keysR, const uint8_t* const* descR,
                                             float mbf, float mb, float* const* uRight,
                                             float* const* depth, int* nmatches);

/* cv::Mat Frame::UnprojectStereo(const int& i)                   Frame.cc:666-680
 * x3D = mRwc * ((u-cx)*z*invfx, (v-cy)*z*invfy, z) + mOw for every keypoint with
 * mvDepth[i] = z > 0 (invfx = 1.0f/fx, Frame.cc:108); the callers are Tracking's
 * UpdateLastFrame / CreateNewKeyFrame / StereoInitialization (Tracking.cc:520-840).
 * Twc: 16 floats row-major, [mRwc | mOw] (the inverse pose).  Rows with z <= 0 are not
 * written; mp (optional) gets i for z > 0 and -1 otherwise (the frame's new map-point
 * slots).  Every pointer is device memory; runs asynchronously on the matcher's stream
 * (ORBmatcher_stream), so a following search on `h` sees the points. */
typedef struct orb_unproject {
    int N;
    const orb_kp* keysUn;        /* mvKeysUn (N) */
    const float* depth;          /* mvDepth (N) */
    const float* Twc;            /* 16 floats: [mRwc | mOw] */
    float fx, fy, cx, cy;
    float* x3D;                  /* out: N x 3 */
    int32_t* mp;                 /* out (may be NULL): i if depth > 0, else -1 */
} orb_unproject;
int Frame_UnprojectStereo_batch_device(ORBmatcher_h h, int count, const orb_unproject* U);

/* void Frame::UndistortKeyPoints()                               Frame.cc:404-430
 * mvKeysUn from mvKeys: when mDistCoef.at<float>(0) == 0 a copy; otherwise every keypoint's pt
 * through cv::undistortPoints(pts, pts, mK, mDistCoef, Mat(), mK) (OpenCV 3.2
 * cvUndistortPoints: double arithmetic, 5 fixed-point iterations; "parity unpinned" at that
 * OpenCV call site) and the rest of each KeyPoint copied.  K: mK row-major;
 * dist: mDistCoef (k1 k2 p1 p2 [k3] [k4 k5 k6]), ndist = 4, 5 or 8.  Pointer space per
 * ORBmatcher_set_device_pointers: device arrays are enqueued on ORBmatcher_stream (batch form)
 * and host arrays are copied and waited for. */
typedef struct orb_undistort {
    int N;
    const orb_kp* keys;          /* mvKeys (N) */
    orb_kp* keysUn;              /* out: mvKeysUn (N); may not alias keys */
    float K[9];                  /* mK */
    float dist[8];               /* mDistCoef, ndist used */
    int ndist;
} orb_undistort;
int Frame_UndistortKeyPoints(ORBmatcher_h h, const orb_undistort* U);
int Frame_UndistortKeyPoints_batch(ORBmatcher_h h, int count, const orb_undistort* U);
/* void Frame::ComputeImageBounds(const cv::Mat&)                    Frame.cc:436-464
 * plus the grid factors the Frame constructors derive from it (Frame.cc:155-156):
 * bounds[0..5] = mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv.
 * With distortion the four image corners go through the UndistortKeyPoints kernel. */
int Frame_ComputeImageBounds(ORBmatcher_h h, int cols, int rows, const float* K, const float* dist, int ndist,
                             float* bounds);

/* void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth), with the depth conversion that
 * Tracking::GrabImageRGBD applies in front of it folded in.  Per keypoint i:
 *   u = (int)keys[i].pt.x, v = (int)keys[i].pt.y   (C++ truncation, as imDepth.at<float>(v, u)
 *                                                   converts its float arguments);
 *   raw = depth pixel (v, u);  d = (float)raw * depthMapFactor when the reference converts, i.e.
 *   when fabs(depthMapFactor - 1.0f) > 1e-5 or depth_type != ORB_DEPTH_F32 (cv::Mat::convertTo(
 *   CV_32F, scale): one float multiply), otherwise d = raw untouched;
 *   d > 0:  depth_out[i] = d, uRight[i] = keysUn[i].pt.x - mbf / d;  otherwise both are -1
 *   (NaN has no depth; +inf gives uRight = keysUn[i].pt.x).
 * The float depth image is never built: N pixels are read, not cols*rows.  One deliberate
 * difference from the reference: a keypoint whose (v, u) lies outside [0, rows) x [0, cols) gets
 * -1 / -1 (the reference would read out of bounds).  ndepth (may be NULL): ndepth[f] = the
 * keypoints of frame f with depth, which Tracking::StereoInitialization tests against 500.
 * Pointer space per ORBmatcher_set_device_pointers, as for Frame_UndistortKeyPoints_batch /
 * ORBmatcher_ComputeStereoMatches_batch: device arrays are enqueued on ORBmatcher_stream and
 * ndepth is read back with the matcher's counts (inside a deferred chain it lands at
 * ORBmatcher_finish); host arrays (keys and the depth image included) are staged, and the
 * results copied back and waited for.  ORB_E_INVALID: N < 0, a null pointer with N > 0, an
 * unknown depth_type, negative cols / rows, step smaller than a row. */
#define ORB_DEPTH_U16 0
#define ORB_DEPTH_F32 1
typedef struct orb_rgbd {
    int N;
    const orb_kp* keys;          /* mvKeys (distorted): picks the depth pixel */
    const orb_kp* keysUn;        /* mvKeysUn: kpU.pt.x of mvuRight */
    const void* depth;           /* imD as the driver loaded it, before convertTo */
    int depth_type;              /* ORB_DEPTH_U16 / ORB_DEPTH_F32 */
    int cols, rows;
    size_t step;                 /* bytes per row */
    float depthMapFactor;        /* Tracking::mDepthMapFactor (already 1/DepthMapFactor, or 1) */
    float mbf;
    float* uRight;               /* out: mvuRight (N), -1 = no depth */
    float* depth_out;            /* out: mvDepth (N), -1 = no depth */
} orb_rgbd;
int Frame_ComputeStereoFromRGBD_batch(ORBmatcher_h h, int count, const orb_rgbd* R, int* ndepth);
/* One frame: the batch form with count = 1. */
int Frame_ComputeStereoFromRGBD(ORBmatcher_h h, const orb_rgbd* R, int* ndepth);

/* New MapPoints from a stereo frame (Tracking::StereoInitialization / CreateNewKeyFrame /
 * UpdateLastFrame, Tracking.cc:520-560, 1025-1080, 837-860): for every keypoint with depth > 0,
 * x3D = UnprojectStereo(i) as above and MapPoint::UpdateNormalAndDepth (MapPoint.cc:331-371)
 * with the frame as the only observation: normal = (x3D - mOw) / |x3D - mOw|, mfMaxDistance =
 * |x3D - mOw| * mvScaleFactors[octave], mfMinDistance = mfMaxDistance / mvScaleFactors[nlevels-1].
 * row[i] = row_base + i (the point's row in the caller's map table) for depth > 0, else -1.
 * Device pointers; enqueued on ORBmatcher_stream. */
typedef struct orb_newpoints {
    int N;
    const orb_kp* keysUn;        /* mvKeysUn (N) */
    const float* depth;          /* mvDepth (N) */
    const float* Twc;            /* 16 floats: [mRwc | mOw] */
    float fx, fy, cx, cy;
    const float* scaleFactors;   /* mvScaleFactors (nlevels) */
    int nlevels;
    int32_t row_base;
    float* x3D;                  /* out: N x 3 */
    int32_t* row;                /* out: N */
    float* normal;               /* out: N x 3 (GetNormal) */
    float* max_dist;             /* out: N (mfMaxDistance) */
    float* min_dist;             /* out: N (mfMinDistance) */
} orb_newpoints;
int MapPoint_CreateStereo_batch_device(ORBmatcher_h h, int count, const orb_newpoints* P);

/* Tracking's bookkeeping between TrackWithMotionModel and SearchLocalPoints: the outliers of
 * the first PoseOptimization are dropped from mvpMapPoints and their points marked seen
 * (Tracking.cc:893-913), the frame's points are skipped by SearchLocalPoints (1146-1161).
 * skip[j] (out, n) = (row[j] < 0: no map point / isBad) or j in cur_mp; then cur_mp[i] = -1
 * where outlier[i].  One launch for all frames; device pointers; synchronous. */
typedef struct orb_localprep {
    int N;
    int32_t* cur_mp;             /* in/out (N): mvpMapPoints as local-map rows */
    const uint8_t* outlier;      /* mvbOutlier (N) after PoseOptimization */
    int n;                       /* local-map rows */
    const int32_t* row;          /* n: < 0 = no map point */
    uint8_t* skip;               /* out: n */
} orb_localprep;
int Tracking_PrepareLocalSearch_batch_device(ORBmatcher_h h, int count, const orb_localprep* P);

/* ======================================================================
 * ORBVocabulary (reference include/ORBVocabulary.h: DBoW2::TemplatedVocabulary<
 * FORB::TDescriptor, FORB>, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h)
 * ====================================================================== */
typedef struct ORBvocabulary_t* ORBvocabulary_h;
int ORBvocabulary_create(ORBvocabulary_h* out);
int ORBvocabulary_destroy(ORBvocabulary_h h);
/* bool loadFromTextFile(const std::string&)  TemplatedVocabulary.h:1338-1424 (host parse).
 * ORB_E_INVALID where the reference returns false (unreadable file, header out of range) or
 * a node names a parent not yet defined.  The trailing line after saveToTextFile's final endl
 * is the reference's undefined behaviour; DESIGN.md §5 states how it is realised. */
int ORBvocabulary_loadFromTextFile(ORBvocabulary_h h, const char* path);
/* m_k, m_L, m_scoring, m_weighting, size of m_nodes (root included), size of m_words */
int ORBvocabulary_info(ORBvocabulary_h h, int* k, int* L, int* scoring, int* weighting, int* n_nodes,
                       int* n_words);
/* One frame's DBoW2::BowVector (std::map<WordId, WordValue>: ascending words) and
 * DBoW2::FeatureVector (as orb_featvec CSR: fv_node ascending, fv_start[n_nodes + 1],
 * fv_feat in insertion order).  Host buffers of capacity `cap` >= N (fv_start: cap + 1). */
typedef struct orb_bow {
    int cap;
    uint32_t* word;
    double* value;
    int n_words;                 /* out */
    uint32_t* fv_node;
    int32_t* fv_start;
    int32_t* fv_feat;
    int n_nodes;                 /* out */
} orb_bow;
/* void transform(const vector<TDescriptor>& features, BowVector& v, FeatureVector& fv,
 *                int levelsup) const                       TemplatedVocabulary.h:1126-1197
 * = Frame::ComputeBoW / KeyFrame::ComputeBoW with levelsup 4 (Frame.cc:395-402).
 * desc: N x 32 descriptors (host).  N <= 4096 per frame (ORB_E_CAPACITY). */
int ORBvocabulary_transform(ORBvocabulary_h h, const uint8_t* desc, int N, int levelsup, orb_bow* out);
/* `count` frames in one launch (one tree walk per descriptor, one assembly per frame). */
int ORBvocabulary_transform_batch(ORBvocabulary_h h, int count, const uint8_t* const* desc, const int* N,
                                  int levelsup, orb_bow* out);
/* void transform(const TDescriptor& feature, WordId& id, WordValue& weight, NodeId* nid,
 *                int levelsup) const, for each of N descriptors  TemplatedVocabulary.h:1217-1256 */
int ORBvocabulary_transform_features(ORBvocabulary_h h, const uint8_t* desc, int N, int levelsup,
                                     uint32_t* word, double* weight, uint32_t* node);
/* double score(const BowVector& a, const BowVector& b) const  (L1Scoring::score,
 * ScoringObject.cpp:21-66) of one query BowVector against `count` candidates given as CSR
 * (candidate c: words/values [cstart[c], cstart[c+1])), as KeyFrameDatabase scores the
 * keyframes sharing words (KeyFrameDatabase.cc:133, 249).  L1_NORM vocabularies only. */
int ORBvocabulary_score(ORBvocabulary_h h, const uint32_t* qw, const double* qv, int nq, int count,
                        const int32_t* cstart, const uint32_t* cw, const double* cv, double* scores);

/* ======================================================================
 * KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc)
 * A device-resident database: every stored keyframe's BowVector lives in device memory and a
 * query scans all of them.  A word's inverted-file list is the live keyframes holding the word in
 * the order of their add calls, so lKFsSharingWords is, in closed form, the sharing keyframes in
 * ascending (index in the query BowVector of the first shared word, add sequence number).
 * All pointers are host pointers.  One mutex per handle (the reference's mMutex).
 * Argument checks come before the device is touched; an otherwise valid call on a NULL handle
 * answers ORB_E_NODEVICE where no device is visible (ORB_E_INVALID otherwise).
 * Two deliberate deviations from the reference:
 *  - DetectRelocalizationCandidates accepts any neighbour with mnRelocQuery == F->mnId (288-289)
 *    and reads its mRelocScore even when that neighbour was not scored for this frame (a value
 *    left by an earlier frame, or the uninitialised member).  Here a neighbour counts only if it
 *    was scored in this query, the loop variant's rule: the call is a function of its inputs.
 *  - the marking fields' initial value 0 aliasing a query id of 0 is not reproduced.
 * ====================================================================== */
typedef struct KeyFrameDatabase_t* KeyFrameDatabase_h;
/* KeyFrameDatabase(const ORBVocabulary&) 32-36.  voc must outlive the database. */
int KeyFrameDatabase_create(ORBvocabulary_h voc, KeyFrameDatabase_h* out);
int KeyFrameDatabase_destroy(KeyFrameDatabase_h h);
/* void add(KeyFrame*) 39-45: id = mnId (>= 0); word/value = mBowVec: words strictly ascending and
 * below the vocabulary's word count; n <= 4096.  An id already present is ORB_E_INVALID (the
 * reference would list it twice; no caller does).  Every add draws a new sequence number. */
int KeyFrameDatabase_add(KeyFrameDatabase_h h, int32_t id, const uint32_t* word, const double* value, int n);
/* `count` keyframes as CSR (start[0] = 0, keyframe i: [start[i], start[i+1])), added in index
 * order (map load, tests).  All of them or none. */
int KeyFrameDatabase_add_batch(KeyFrameDatabase_h h, int count, const int32_t* id, const int32_t* start,
                               const uint32_t* word, const double* value);
/* void erase(KeyFrame*) 47-67; an absent id is ORB_OK.  void clear() 69-73. */
int KeyFrameDatabase_erase(KeyFrameDatabase_h h, int32_t id);
int KeyFrameDatabase_clear(KeyFrameDatabase_h h);
/* live keyframes and the BowVector entries they hold */
int KeyFrameDatabase_size(KeyFrameDatabase_h h, int* n_keyframes, long long* n_entries);
/* GetBestCovisibilityKeyFrames(10) of keyframe `id` as the accumulation step reads it (160, 277):
 * the first n <= 10 of mvpOrderedConnectedKeyFrames.  Replaces the previous list (n = 0 drops it);
 * ids need not be in the database.  The list belongs to the keyframe, not to its database entry:
 * it may be set before add (LocalMapping updates connections before LoopClosing adds) and
 * survives erase and clear. */
int KeyFrameDatabase_set_covisibles(KeyFrameDatabase_h h, int32_t id, int n, const int32_t* ids);

typedef struct orb_kfdb_query {
    int nq;                      /* the query BowVector: nq <= 4096 words, strictly ascending */
    const uint32_t* word;
    const double* value;
    int n_exclude;               /* loop: pKF->GetConnectedKeyFrames() (82); reloc: ignored */
    const int32_t* exclude;
    float minScore;              /* loop only */
} orb_kfdb_query;
typedef struct orb_kfdb_result {
    int cap;                     /* capacity of cand */
    int32_t* cand;               /* out: candidates in the reference's order */
    int n_cand;                  /* out */
    /* stage outputs, each pointer may be NULL: the scored subset (words > minCommonWords) in
     * lKFsSharingWords order, capacity cap_scored */
    int cap_scored;
    int32_t* scored_id;
    int32_t* scored_words;       /* mnLoopWords / mnRelocWords */
    float* scored_score;         /* mLoopScore / mRelocScore */
    float* scored_acc;           /* accScore of the entries that reached lScoreAndMatch, else NaN */
    int n_scored, n_sharing, maxCommonWords, minCommonWords;   /* out */
    float bestAccScore;          /* out (its initial value where there is no candidate) */
} orb_kfdb_result;
/* vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) 76-197.
 * ORB_E_CAPACITY when n_cand > cap or n_scored > cap_scored: the counts needed are set and
 * nothing is written past a capacity.  L1_NORM vocabularies only (ORB_E_INVALID otherwise). */
int KeyFrameDatabase_DetectLoopCandidates(KeyFrameDatabase_h h, const orb_kfdb_query* q, orb_kfdb_result* r);
/* vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F) 199-309 */
int KeyFrameDatabase_DetectRelocalizationCandidates(KeyFrameDatabase_h h, const orb_kfdb_query* q,
                                                    orb_kfdb_result* r);
/* `count` frames against one database state in one launch set, one synchronisation */
int KeyFrameDatabase_DetectRelocalizationCandidates_batch(KeyFrameDatabase_h h, int count,
                                                          const orb_kfdb_query* q, orb_kfdb_result* r);
/* Measurement (no reference counterpart): ms3 = {share count and selection, scoring, whole call}
 * of the last timed query; the first two are HIP-event times, the third is host wall time. */
int KeyFrameDatabase_enable_timing(KeyFrameDatabase_h h, int on);
int KeyFrameDatabase_last_timings(KeyFrameDatabase_h h, float* ms3);

/* ======================================================================
 * Map: the keyframe <-> map-point observation relation in device memory, and the two counting
 * functions over it: Tracking::UpdateLocalMap (src/Tracking.cc:1195-1339) and
 * KeyFrame::UpdateConnections (src/KeyFrame.cc).
 * Per live keyframe the handle stores one row: mp[slot] = the map-point id of
 * KeyFrame::mvpMapPoints[slot] (-1 = none) and observed[slot] = whether that point's
 * mObservations holds (this keyframe, slot).  The two differ for a while in the reference:
 * Tracking::CreateNewKeyFrame copies the frame's map points into the keyframe at once,
 * LocalMapping::ProcessNewKeyFrame adds the observations later.
 *  - The observed rule: the vote (UpdateLocalKeyFrames, UpdateConnections) reads observed slots
 *    only; UpdateLocalPoints reads every slot.
 *  - The id-order rule: where the reference iterates a std::map<KeyFrame*, int> or a
 *    std::set<KeyFrame*> (keyframeCounter, KFcounter, mspChildrens) its order is the keyframes'
 *    address order; ascending keyframe id stands in for it everywhere here.
 * Map-point ids are the rows of the caller's map-point table (non-negative int32, as
 * orb_newpoints.row); keyframe ids are mnId (non-negative, dense: two tables are indexed by them).
 * Mutations are host calls on host pointers: they update a host mirror, and the next query
 * uploads the changed rows and rebuilds the inverse index (map point -> observing keyframes) on
 * the device.  One mutex per handle stands for the map's and the keyframes' mutexes; queries from
 * several matchers are serialised by it and ordered on the device by an event.
 * Argument checks come before the device is touched; an otherwise valid call on a NULL handle
 * answers ORB_E_NODEVICE where no device is visible (ORB_E_INVALID otherwise).
 * ====================================================================== */
typedef struct Map_t* Map_h;
int Map_create(Map_h* out);
int Map_destroy(Map_h h);
/* void Map::clear() */
int Map_clear(Map_h h);
/* live keyframes, the slots of their rows, and the observed slots among them */
int Map_size(Map_h h, int* n_keyframes, long long* n_slots, long long* n_observations);
/* Map::AddKeyFrame with the keyframe's mvpMapPoints (Tracking::CreateNewKeyFrame, KeyFrame's
 * constructor): N <= 4096 slots, mp[slot] >= 0 or -1, observed[slot] (NULL = all 1).
 * ORB_E_INVALID: N > 4096, an id already present, a map point held twice in the row. */
int Map_AddKeyFrame(Map_h h, int32_t id, int N, const int32_t* mp, const uint8_t* observed);
/* Sparse updates of one row, for KeyFrame::AddMapPoint / EraseMapPointMatch /
 * ReplaceMapPointMatch and MapPoint::AddObservation / EraseObservation: slot[k] takes mp[k]
 * (-1 empties it) with observed[k] (NULL = all 1).  ORB_E_INVALID: an unknown id, a slot outside
 * the row or named twice, a point that the row would then hold twice. */
int Map_SetMapPointMatches(Map_h h, int32_t id, int count, const int32_t* slot, const int32_t* mp,
                           const uint8_t* observed);
/* MapPoint::SetBadFlag (MapPoint.cc): every slot that holds `mp` is emptied. */
int Map_EraseMapPoint(Map_h h, int32_t mp);
/* MapPoint::Replace (MapPoint.cc), per keyframe that observes `mp`: the slot takes `by`
 * (observed), unless `by` is already in that row, in which case the slot is emptied.  A slot that
 * holds `mp` without the observation is emptied (the reference leaves a bad point there, which
 * every reader skips). */
int Map_ReplaceMapPoint(Map_h h, int32_t mp, int32_t by);
/* KeyFrame::SetBadFlag: erased keyframes are the reference's bad keyframes: they never vote, are
 * never neighbours, and their storage is reused.  An absent id is ORB_OK. */
int Map_EraseKeyFrame(Map_h h, int32_t id);
/* The neighbour record UpdateLocalKeyFrames reads: ids10 = the first n10 <= 10 of
 * mvpOrderedConnectedKeyFrames (GetBestCovisibilityKeyFrames(10)), parent = mpParent's id or -1,
 * children = mspChildrens (any order; kept in ascending id order, the id-order rule).  Forwarded
 * from the places that call KeyFrameDatabase_set_covisibles, and from AddChild / EraseChild /
 * ChangeParent.  Ids not (or no longer) in the handle are skipped at query time, as bad keyframes
 * are.  ORB_E_INVALID: `id` is not in the handle. */
int Map_SetNeighbours(Map_h h, int32_t id, int n10, const int32_t* ids10, int32_t parent, int nchild,
                      const int32_t* children);

/* void KeyFrame::UpdateConnections() (KeyFrame.cc): the vote over the keyframe's own row (every
 * slot >= 0; each point's observers counted, the keyframe itself excluded; the observed rule).
 * counter_* = KFcounter: every keyframe with count > 0 in ascending id (the id-order rule).
 * ordered_* = mvpOrderedConnectedKeyFrames / mvOrderedWeights: the entries with count >= 15, or
 * where there is none the single maximum (the first strict maximum in ascending id), sorted by
 * descending (weight, id): among equal weights the larger id comes first (the reference sorts
 * pair<int, KeyFrame*> ascending and pushes to the front).  ORB_E_CAPACITY when n_counter >
 * cap_counter or n_ordered > cap_ordered: the counts needed are set and nothing is written past
 * a capacity; call again.  AddConnection on the other keyframes, the first-connection parent and
 * the forwards (Map_SetNeighbours, KeyFrameDatabase_set_covisibles) are the adapter's.
 * Host pointers; synchronous; runs on the handle's own stream. */
typedef struct orb_connections {
    int cap_counter;
    int32_t* counter_id;         /* out */
    int32_t* counter_n;          /* out */
    int cap_ordered;
    int32_t* ordered_id;         /* out */
    int32_t* ordered_w;          /* out */
    int n_counter, n_ordered;    /* out */
} orb_connections;
int KeyFrame_UpdateConnections(Map_h h, int32_t id, orb_connections* r);
/* `count` keyframes against one map state in one launch set (LoopClosing::CorrectLoop) */
int KeyFrame_UpdateConnections_batch(Map_h h, int count, const int32_t* id, orb_connections* r);

/* void Tracking::UpdateLocalMap()                              Tracking.cc:1195-1339
 * UpdateLocalKeyFrames (1237-1339): every map point of the frame that is not bad votes for the
 * keyframes observing it (a point held by two keypoints votes twice; the observed rule); bad
 * points are cleared from cur_mp.  local_kf = the voted keyframes in ascending id (the id-order
 * rule), ref_kf = the first strict maximum in that order; then for each voted keyframe in order,
 * while the list holds at most 80: the first of its best-10 covisibles that is live and not yet
 * listed, the first such child, and the parent if live and not yet listed -- after which the
 * whole loop ends (the reference's break sits in the outer loop's body).  An empty vote gives
 * n_kf = 0, ref_kf = -1, n_pt = 0 and leaves every output array but cur_mp untouched.
 * UpdateLocalPoints (1214-1235): the rows of local_kf in list order, slots in index order, every
 * slot >= 0 that is not bad regardless of `observed`, first occurrence kept: local_mp.
 * Then cur_row[i] = the local row of cur_mp[i] or -1 (what orb_localprep.cur_mp and
 * ORBmatcher_SearchLocalPoints_batch expect), row[j] = local_mp[j], and with device pointers the
 * global table's rows gathered into pos / desc / observations / max_dist / min_dist / normal with
 * skip[j] = 0 (all seven or none; they are the arrays of the frame's orb_localmap).  With device
 * pointers the rows [n_pt, pt_cap) get row = -1 and skip = 1, so a deferred chain passes
 * orb_localmap.n = orb_localprep.n = pt_cap without knowing n_pt.
 * table: the caller's global map-point table; n = its rows, skip = isBad(); pos .. normal are
 * read by the gather only.  NULL: no point is bad.
 * Runs on ORBmatcher_stream(h); pointer space per ORBmatcher_set_device_pointers (counts and
 * this struct stay host).  On a deferred matcher the call joins the chain and n_kf / ref_kf /
 * n_pt are written when ORBmatcher_finish returns: U must stay in place until then.
 * Capacity: nothing is written past kf_cap / pt_cap and the counts needed are reported; the
 * synchronous forms return ORB_E_CAPACITY, a deferred caller compares n_kf > kf_cap and n_pt >
 * pt_cap after finish and queues the step again with larger arrays.  N <= 4096. */
typedef struct orb_localupdate {
    int N;
    int32_t* cur_mp;             /* in/out (N): mCurrentFrame.mvpMapPoints as global ids */
    const orb_localmap* table;
    int kf_cap, pt_cap;
    int32_t* local_kf;           /* out (kf_cap): mvpLocalKeyFrames as ids */
    int32_t* local_mp;           /* out (pt_cap): mvpLocalMapPoints as global ids */
    int32_t* cur_row;            /* out (N) */
    int32_t* row;                /* out (pt_cap), may be NULL */
    float* pos;                  /* gather outputs (pt_cap rows), device pointers only */
    uint8_t* desc;
    int* observations;
    float* max_dist;
    float* min_dist;
    float* normal;
    uint8_t* skip;
    int32_t n_kf, ref_kf, n_pt, reserved;   /* out */
} orb_localupdate;
int Tracking_UpdateLocalMap_batch(ORBmatcher_h h, Map_h map, int count, orb_localupdate* U);
/* Measurement (no reference counterpart): HIP-event times (ms) of the last timed
 * Tracking_UpdateLocalMap_batch (of its last chunk where the batch ran in several):
 * ms5 = {index rebuild (-1: nothing had changed), vote, keyframe selection, local points,
 * remap + gather}.  Waits for that work. */
int Map_enable_timing(Map_h h, int on);
int Map_last_timings(Map_h h, float* ms5);

/* ---- LocalMapping::KeyFrameCulling and MapPointCulling over the Map handle -----------------
 * The per-slot key attributes of one keyframe row, forwarded once from the KeyFrame constructor:
 * octave[i] = mvKeysUn[i].octave; uRight = mvuRight (NULL: every observation is monocular; else
 * slot i is stereo when uRight[i] >= 0, and its observation counts 2 in MapPoint::nObs,
 * MapPoint.cc AddObservation / EraseObservation); depth = mvDepth and thDepth = mThDepth (NULL: no
 * slot is far; else slot i is far when depth[i] > thDepth || depth[i] < 0, LocalMapping.cc
 * KeyFrameCulling).  The handle keeps one byte of octave and the two bits per slot; they follow
 * the row through repacks, and a keyframe whose keys were never set reads as octave 0,
 * monocular, not far.  N must equal the row's slot count.  ORB_E_INVALID: an unknown id, another
 * N.  Only octave is dereferenced before the handle is looked at. */
int Map_SetKeyFrameKeys(Map_h h, int32_t id, int N, const uint8_t* octave, const float* uRight,
                        const float* depth, float thDepth);

/* void LocalMapping::KeyFrameCulling()                          LocalMapping.cc
 * cand = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames() as ids, examined one after another.
 * Per candidate: id 0 or an id not live in the handle is skipped (verdict 3).  Over the row's
 * slots that hold a point that is not bad (bad[] or gone bad earlier in this call), and unless
 * monocular that are not far: nMPs counts them; a point with Observations() > 3 (MapPoint::nObs:
 * 2 per stereo observation, 1 per monocular one) whose observers other than the candidate, with
 * octave <= the slot's octave + 1, number at least 3 (the count saturates there, so the order
 * inside mObservations is not observable) adds to nRedundant.  nRedundant > 0.9 * nMPs in double
 * makes the candidate redundant: with not_erase (KeyFrame::mbNotErase) that only sets mbToBeErased
 * (verdict 2, nothing changes); otherwise KeyFrame::SetBadFlag (verdict 1): in slot order
 * MapPoint::EraseObservation of every observed slot takes 2 or 1 off the point's nObs, and a point
 * left with nObs <= 2 runs MapPoint::SetBadFlag -- it leaves every row and is reported in bad_mp,
 * in cull order and within a cull in ascending slot of the culled row.  Every later candidate is
 * counted against the state the earlier culls left; nMPs / nRedundant are the counts at the moment
 * the candidate was examined.
 * apply != 0: on ORB_OK the handle erases the culled keyframes and the reported points, as
 * Map_EraseKeyFrame / Map_EraseMapPoint would; apply == 0 leaves the handle as it was.  The
 * spanning-tree repair and connection bookkeeping of KeyFrame::SetBadFlag, mpRefKF of the points
 * and KeyFrameDatabase_erase stay with the adapter.
 * ORB_E_CAPACITY when n_bad > cap_bad: n_bad is set, nothing is written past cap_bad and nothing
 * is applied; call again.  ORB_E_INVALID: n < 0, a candidate named twice, a missing array.
 * Host pointers; synchronous; runs on the handle's own stream. */
typedef struct orb_kfcull {
    int n;
    const int32_t* cand;         /* n */
    const uint8_t* not_erase;    /* n, may be NULL */
    int monocular;               /* LocalMapping::mbMonocular */
    const uint8_t* bad;          /* the map-point table's isBad() flags (nbad), may be NULL */
    int nbad;
    int cap_bad;
    int apply;
    int32_t* nMPs;               /* out (n) */
    int32_t* nRedundant;         /* out (n) */
    int32_t* verdict;            /* out (n): 0 kept, 1 SetBadFlag, 2 mbToBeErased, 3 skipped */
    int32_t* bad_mp;             /* out (cap_bad) */
    int n_bad;                   /* out */
} orb_kfcull;
int LocalMapping_KeyFrameCulling(Map_h h, orb_kfcull* r);

/* void LocalMapping::MapPointCulling()                          LocalMapping.cc
 * Per point of mlpRecentAddedMapPoints, independently, the first rule that holds: isBad() (bad[])
 * -> verdict 1 (dropped); GetFoundRatio() = float(found) / visible < 0.25f -> 2 (SetBadFlag);
 * (int)cur_kf - (int)first_kf >= 2 && Observations() <= cnThObs (2 when monocular, else 3) -> 3
 * (SetBadFlag); the same difference >= 3 -> 4 (dropped); else 0 (kept).  observations (may be
 * NULL) = MapPoint::Observations() as the handle counts it; an id the handle never saw has 0.
 * apply != 0: the points with verdict 2 or 3 are erased as Map_EraseMapPoint would.
 * ORB_E_INVALID: n < 0, mp[i] < 0, visible[i] <= 0, a missing array.  Host pointers; synchronous. */
typedef struct orb_pointcull {
    int n;
    const int32_t* mp;           /* n: map-point ids */
    const int32_t* first_kf;     /* n: mnFirstKFid */
    const int32_t* found;        /* n: mnFound */
    const int32_t* visible;      /* n: mnVisible */
    const uint8_t* bad;          /* isBad() flags (nbad), may be NULL */
    int nbad;
    int32_t cur_kf;              /* mpCurrentKeyFrame->mnId */
    int monocular;
    int apply;
    int32_t* verdict;            /* out (n) */
    int32_t* observations;       /* out (n), may be NULL */
} orb_pointcull;
int LocalMapping_MapPointCulling(Map_h h, orb_pointcull* r);

/* ---- LoopClosing's map correction over the Map handle -------------------------------------
 * The two steps of the loop-closing thread that move the map: the first half of
 * LoopClosing::CorrectLoop and the tail of LoopClosing::RunGlobalBundleAdjustment
 * (src/LoopClosing.cc).  Both work on the caller's tables: the keyframe pose table Tcw
 * (n_kf_rows x 16 floats, row-major, indexed by mnId; every id the handle has seen must be below
 * n_kf_rows) and the map-point table indexed by the map-point row, as
 * Tracking_UpdateLocalMap_batch gathers from it.
 * Pointer space: every array marked (table) is in the pointer space of
 * ORBmatcher_set_device_pointers(h); lists, counts, the Sim3 arrays and the structs are host.
 * Both calls run on ORBmatcher_stream(h), hold the map handle's lock and return when their
 * results are in place.  A matcher in deferred mode answers ORB_E_INVALID.
 * Arithmetic: a cv::Mat product is one cv::gemm (float operands, the sum over k ascending in
 * double, one rounding to float); SetPose(Tcw) forms Rwc = Rcw^T and Ow = -Rwc * tcw as a gemm with
 * alpha -1; g2o::Sim3(R, t, 1) widens to double and takes Eigen's Quaterniond(Matrix3d) without
 * normalising; Sim3 products, inverse and map are g2o's (sim3.h); toCvMat is one cast per entry.
 * ORB_E_INVALID, before any table is written: a null required array, a listed keyframe that is not
 * live in the handle or is named twice, an id >= n_kf_rows, a non-finite Scw or s <= 0, a cycle in
 * the children relation of Map_SetNeighbours.  A call with a NULL handle answers ORB_E_NODEVICE
 * where no device is visible (ORB_E_INVALID otherwise). */
typedef struct orb_pointtable {
    int n;                       /* rows */
    float* pos;                  /* (table) n x 3, in/out */
    float* normal;               /* (table) n x 3, in/out (CorrectLoop) */
    float* max_dist;             /* (table) n, in/out (CorrectLoop) */
    float* min_dist;             /* (table) n, in/out (CorrectLoop) */
    const uint8_t* bad;          /* (table) n: isBad(), may be NULL */
    const int32_t* ref_kf;       /* (table) n: mpRefKF's id, -1 = none */
} orb_pointtable;

/* void LoopClosing::CorrectLoop(), from CorrectedSim3[mpCurrentKF] = mg2oScw to the end of the
 * loop over CorrectedSim3.  The listed keyframes are processed in ascending id (the id-order rule
 * for the KeyFrameAndPose map), whatever order kf[] has.
 * 1. Per listed keyframe i, from the old poses: NonCorrected[i] = Sim3(Riw, tiw, 1);
 *    Corrected[cur] = Scw, otherwise Tic = Tiw * Twc(cur), Corrected[i] = Sim3(Ric, tic, 1) * Scw.
 * 2. Every point held in any slot of a listed keyframe (observed or not) that is not bad is
 *    corrected once, by the listed keyframe of lowest id that holds it; corrected_ref[p] takes that
 *    id (mnCorrectedReference).  Other rows of corrected_ref are untouched.  A held id >= pts.n is
 *    skipped.
 * 3. pos[p] = (float) Corrected[k]^-1.map(NonCorrected[k].map((double) pos[p])).
 * 4. MapPoint::UpdateNormalAndDepth of each corrected point with the new position over its
 *    observations in the handle, taken in ascending keyframe id.  The camera centre of an observer
 *    (and of ref_kf[p]) comes from its corrected pose when it is a listed keyframe processed before
 *    the corrector, else from its old pose.  ref_scale = scale_factors[octave of ref_kf's observing
 *    slot] (Map_SetKeyFrameKeys), ref_scale_top = scale_factors[nlevels - 1].  A point without
 *    observations keeps normal / max_dist / min_dist.  So does a point whose ref_kf is -1 or not
 *    among its observers, or whose octave is >= nlevels; those count in n_ref_missing (the
 *    reference would read keypoint 0 there).
 * 5. Tcw[i] = [R(Corrected[i]) | t * (1 / s); 0 0 0 1] for every listed i.
 * KeyFrame::UpdateConnections of the listed keyframes stays with
 * KeyFrame_UpdateConnections_batch; the relation is not changed here. */
typedef struct orb_loopcorrect {
    int nkf;
    const int32_t* kf;           /* nkf: mvpCurrentConnectedKFs with the current keyframe */
    int32_t cur_kf;
    const double* Scw;           /* 8: mg2oScw as q xyzw, t, s (the layout of essgraph_problem) */
    int nlevels;
    const float* scale_factors;  /* nlevels: mvScaleFactors */
    int n_kf_rows;
    float* Tcw;                  /* (table) n_kf_rows x 16, in/out */
    orb_pointtable pts;
    int32_t* corrected_ref;      /* (table) pts.n, in/out */
    double* CorrectedSim3;       /* out nkf x 8, in the order of kf[] */
    double* NonCorrectedSim3;    /* out nkf x 8, in the order of kf[] */
    int32_t n_corrected, n_ref_missing;   /* out */
} orb_loopcorrect;
int LoopClosing_CorrectLoop(ORBmatcher_h h, Map_h map, orb_loopcorrect* C);

/* void LoopClosing::RunGlobalBundleAdjustment(nLoopKF), the write-back after the optimisation:
 * the spanning tree is walked breadth first from `origins` (mvpKeyFrameOrigins) over the handle's
 * children; ids not live in the handle are skipped, as bad keyframes are.  A child without
 * kf_in_gba takes TcwGBA[child] = (Tcw[child] * Twc[parent]) * TcwGBA[parent] (two gemms, the old
 * Tcw) and counts as in the BA from then on; a child with kf_in_gba keeps its row.  Every reached
 * keyframe then gets TcwBefGBA = Tcw and Tcw = TcwGBA; unreached keyframes are untouched.  An
 * origin that is live but not in the BA is ORB_E_INVALID.
 * Every point that is not bad: with mp_in_gba, pos = posGBA; otherwise with r = ref_kf[p] reached,
 * Xc = Rcw_bef[r] * X + tcw_bef[r], pos = Rwc[r] * Xc + Ow[r] from SetPose(TcwGBA[r]) (one gemm
 * each); with r = -1 or unreached the point is untouched.  No UpdateNormalAndDepth follows.
 * n_kf_propagated = the keyframes that took a propagated pose, depth = the longest chain of them
 * (the number of dependent steps run), n_mp_gba / n_mp_moved = the points of the two kinds. */
typedef struct orb_gbaapply {
    int norigins;
    const int32_t* origins;
    int n_kf_rows;
    float* TcwGBA;               /* (table) n_kf_rows x 16: read where kf_in_gba, written where propagated */
    const uint8_t* kf_in_gba;    /* (table) n_kf_rows: mnBAGlobalForKF == nLoopKF */
    float* Tcw;                  /* (table) n_kf_rows x 16, in/out */
    orb_pointtable pts;          /* pos in/out, bad, ref_kf; the other arrays are not read */
    const float* posGBA;         /* (table) pts.n x 3: mPosGBA */
    const uint8_t* mp_in_gba;    /* (table) pts.n: mnBAGlobalForKF == nLoopKF */
    float* TcwBefGBA;            /* (table) out n_kf_rows x 16, may be NULL: the rows of reached keyframes */
    uint8_t* kf_done;            /* (table) out n_kf_rows, may be NULL: 1 = reached */
    int32_t n_kf_propagated, n_mp_gba, n_mp_moved, depth;   /* out */
} orb_gbaapply;
int LoopClosing_ApplyGlobalBA(ORBmatcher_h h, Map_h map, orb_gbaapply* G);

/* ---- LocalMapping::SearchInNeighbors over the Map handle ----------------------------------
 * void LocalMapping::SearchInNeighbors()                          LocalMapping.cc:454-553
 * Every ORBmatcher::Fuse(pKF, vpMapPoints, th) call of one SearchInNeighbors (ORBmatcher.cc:825-975),
 * the MapPoint::Replace / AddObservation / AddMapPoint they run, and the update of the current
 * keyframe's points that follows (543-552), as one call that is exact across the targets: a point
 * that survives a Replace meets the next target with its recomputed descriptor, and isBad(),
 * IsInKeyFrame(pKF) and Observations() are read on the state the earlier passes left.
 *
 * cur / cur_kf = mpCurrentKeyFrame; target[] / target_id[] = vpTargetKFs in the reference's order
 * (the caller chooses them; a keyframe may be listed more than once, cur_kf may not be listed).
 * kf_desc[id] = mDescriptors of every keyframe live in the handle (row slots x 32) and Ow[id] =
 * GetCameraCenter(), indexed by mnId below n_kf_rows.  The map-point table has rows = map-point ids.
 * Observations() is the handle's count: 2 per stereo slot, 1 per monocular slot (Map_SetKeyFrameKeys).
 *
 * 1. Forward passes.  The point list is the current keyframe's row when the call starts.  For each
 *    target in list order a point is skipped when it is -1, bad (bad[] or replaced earlier in this
 *    call) or held by an observed slot of the target's row.  The selection per point is that of
 *    ORBmatcher_Fuse with the point's current descriptor.
 * 2. The mutations of a pass run in point order (951-971): the chosen slot holds q that is not bad:
 *    Observations(q) > Observations(p) ? p->Replace(q) : q->Replace(p); it holds a q with bad[q]:
 *    nothing; it is empty: AddObservation + AddMapPoint.  All three count in nfused.  Replace is
 *    exactly Map_ReplaceMapPoint.
 * 3. Every point that survived a Replace gets ComputeDistinctiveDescriptors over its observers in
 *    ascending keyframe id (the median and tie rule of MapPoint_Update_batch), before the next pass.
 * 4. Backward pass.  Candidates: the targets in list order, their slots in index order, every held
 *    point that is not bad and not yet listed (mnFuseCandidateForKF), on the state after the forward
 *    passes; one Fuse pass into the current keyframe, then step 3.
 * 5. Every point the current keyframe's row then holds that is not bad: ComputeDistinctiveDescriptors
 *    and UpdateNormalAndDepth over its observers in ascending id with Ow, ref_kf, the octave of
 *    ref_kf's observing slot and scale_factors.  A point whose ref_kf is -1, not among its observers
 *    or whose octave is >= nlevels keeps normal / max_dist / min_dist and counts in n_ref_missing, as
 *    in LoopClosing_CorrectLoop step 4.  KeyFrame::UpdateConnections stays KeyFrame_UpdateConnections.
 *
 * nfused[t] = the return value of pass t (t = ntargets: the backward pass).  ops = the mutations in
 * execution order, six int32 each: (pass, kind, a, b, kf, idx) with kind 1 = point a added at slot
 * idx of keyframe kf (b = -1), 2 = a->Replace(b) decided at slot idx of kf (the adapter also moves
 * mnFound / mnVisible: IncreaseFound / IncreaseVisible of MapPoint::Replace), 3 = point a met the
 * bad point b there.  updated = the ids whose desc / normal / max_dist / min_dist / bad rows were
 * written, ascending.  Table rows are written on ORB_OK only; replaced points get bad = 1.
 * apply != 0: on ORB_OK the handle takes the mutations; apply == 0 leaves it as it was.
 * ORB_E_CAPACITY when n_ops > cap_ops or n_updated > cap_updated: both counts are set, nothing is
 * written and nothing is applied.  ORB_E_INVALID, before the device is touched: a missing array, a
 * negative count, an id that is not live in the handle or >= n_kf_rows, cur_kf among the targets, a
 * NULL kf_desc of a live keyframe, an orb_frame whose N is not the row's size or with an octave
 * outside [0, nlevels), a row of cur or of a target with a held but unobserved slot or a held id >=
 * n, a device-pointer or deferred matcher.  Handles are looked at last: a well-formed call with a
 * NULL handle answers ORB_E_NODEVICE where no device is visible (ORB_E_INVALID otherwise).
 * Host pointers; runs on ORBmatcher_stream(h), holds the map handle's lock, synchronous. */
typedef struct orb_searchneigh {
    int32_t cur_kf;
    const orb_frame* cur;
    int ntargets;
    const int32_t* target_id;    /* ntargets */
    const orb_frame* target;     /* ntargets */
    float th;                    /* 3.0 in the reference */
    float logScaleFactor;
    int n_kf_rows;
    const uint8_t* const* kf_desc; /* n_kf_rows pointers */
    const float* Ow;             /* n_kf_rows x 3 */
    int nlevels;
    const float* scale_factors;  /* nlevels */
    int n;                       /* map-point table rows */
    const float* pos;            /* n x 3 */
    uint8_t* desc;               /* n x 32, in/out */
    float* normal;               /* n x 3, in/out */
    float* max_dist;             /* n, in/out */
    float* min_dist;             /* n, in/out */
    uint8_t* bad;                /* n, in/out */
    const int32_t* ref_kf;       /* n */
    int apply, cap_ops, cap_updated;
    int32_t* nfused;             /* out ntargets + 1 */
    int32_t* ops;                /* out cap_ops x 6 */
    int32_t* updated;            /* out cap_updated */
    int32_t n_ops, n_updated, n_ref_missing;   /* out */
} orb_searchneigh;
int LocalMapping_SearchInNeighbors(ORBmatcher_h h, Map_h map, orb_searchneigh* S);
/* With Map_enable_timing on: ms5 = projection, match (summed over the passes), descriptor
 * recomputation (summed), final update (HIP events on the matcher's stream) and the host replay
 * (wall clock) of the last LocalMapping_SearchInNeighbors; ORB_E_INVALID before the first one. */
int LocalMapping_SearchInNeighbors_last_timings(Map_h map, float* ms5);

/* ---- LoopClosing::SearchAndFuse over the Map handle ----------------------------------------
 * The "Start Loop Fusion" block of LoopClosing::CorrectLoop and
 * void LoopClosing::SearchAndFuse(const KeyFrameAndPose& CorrectedPosesMap)     LoopClosing.cc
 * Every ORBmatcher::Fuse(pKF, cvScw, mvpLoopMapPoints, 4, vpReplacePoints) call of one loop closure
 * (ORBmatcher.cc:977-1100) with the vpReplacePoints[i]->Replace(mvpLoopMapPoints[i]) that follow each
 * of them, as one call that is exact across the keyframes: a Replace after one keyframe makes points
 * bad, moves observations and, through ComputeDistinctiveDescriptors at the end of MapPoint::Replace,
 * changes the descriptor the survivor is matched with in the next keyframe.
 *
 * kf[] / frame[] / Scw[] = the keyframes of CorrectedSim3 with their corrected Sim3 (q xyzw, t, s:
 * the CorrectedSim3 output of LoopClosing_CorrectLoop), in any order; the passes run in ascending
 * keyframe id (the id-order rule for the pointer-keyed KeyFrameAndPose map).  The frames carry keysUn,
 * desc, N, grid bounds, intrinsics and scaleFactors; Tcw is not read and may be NULL.  loop_pts =
 * mvpLoopMapPoints as map-point ids (-1 = NULL, skipped).  cur_kf / matched[] = mpCurrentKF and
 * mvpCurrentMatchedPoints as ids, one per slot of its row (-1 = NULL); matched == NULL skips step 0.
 * kf_desc[id] = mDescriptors of every keyframe live in the handle, by mnId below n_kf_rows.  The
 * map-point table has rows = map-point ids; pos, normal, max_dist and min_dist are read only (nothing
 * in this part of the reference moves them), desc and bad are in/out.
 *
 * 0. For each slot i of cur_kf's row in index order with L = matched[i] >= 0: the slot holds c: c == L
 *    is nothing (Replace returns at once), otherwise c->Replace(L) (kind 2).  The slot is empty and L is
 *    not in the row: AddMapPoint + AddObservation + ComputeDistinctiveDescriptors(L) (kind 1).
 *    Deliberate difference: the slot is empty and another slot of the row already holds L: the entry
 *    is skipped and counted in n_matched_skipped (the reference would leave slot i holding L without an
 *    observation, a state the handle refuses, see Map_SetMapPointMatches).
 * 1. Per listed keyframe: cvScw = Converter::toCvMat(g2oScw) (R = q.toRotationMatrix() in double, the
 *    entries (float)(s * R_ij) and (float)t_i), then scw, Rcw, tcw, Ow as ORBmatcher_Fuse_Sim3 takes them.
 * 2. skip[i] = loop_pts[i] < 0 || bad (bad[] or replaced earlier in this call) || held by the
 *    keyframe's row, taken when the pass starts (spAlreadyFound = pKF->GetMapPoints()).
 * 3. The selection per point is that of ORBmatcher_Fuse_Sim3 with the point's current descriptor.
 * 4. In point order: the chosen slot holds q that is not bad: vpReplacePoint[i] = q; it holds a bad q:
 *    nothing (kind 3); it is empty: AddObservation + AddMapPoint (kind 1; a later point of the pass that
 *    chooses that keypoint finds this one there).  All three count in nfused.
 * 5. After the pass, in point order: vpReplacePoint[i]->Replace(loop_pts[i]) (kind 2), exactly
 *    Map_ReplaceMapPoint.  A q that an earlier Replace of this loop already made bad is replaced again
 *    as in the reference: nothing moves, the op is logged and the survivor's descriptor is recomputed.
 * 6. Every survivor of step 0 / of a pass gets ComputeDistinctiveDescriptors over its observers in
 *    ascending keyframe id (the median and tie rule of MapPoint_Update_batch) before the next pass.
 *
 * nfused[k] = the return value of the Fuse into kf[k].  ops = the mutations in execution order, six
 * int32 each: (pass, kind, a, b, kf, idx) with pass = the index into kf[] (-1: step 0) and the kinds
 * of orb_searchneigh: 1 = point a added at slot idx of keyframe kf (b = -1), 2 = a->Replace(b) decided
 * at that slot (IncreaseFound / IncreaseVisible of MapPoint::Replace are the adapter's), 3 = point a met
 * the bad point b there.  updated = the ids whose desc or bad row was written, ascending.  Table rows
 * are written on ORB_OK only; replaced points get bad = 1.  apply != 0: on ORB_OK the handle takes the
 * mutations; apply == 0 and every failure leave the handle and the table as they were.
 * ORB_E_CAPACITY when n_ops > cap_ops or n_updated > cap_updated: both counts are set, nothing is
 * written and nothing is applied.  ORB_E_INVALID, before the device is touched: a missing array, a
 * negative count, a listed id that is not live in the handle, >= n_kf_rows or named twice, loop_pts
 * holding an id twice or an id >= n, a matched[] id >= n or bad when the call starts, an orb_frame
 * whose N is not the row's size or with an octave outside [0, nlevels), nmatched different from
 * cur_kf's row size, a row of a listed keyframe (or of cur_kf in step 0) with a held but unobserved
 * slot or a held id >= n, a NULL kf_desc of a live keyframe, a non-finite Scw or s <= 0, a
 * device-pointer or deferred matcher.  What needs no handle is checked first and the handles are
 * looked at last: a well-formed call with a NULL handle answers ORB_E_NODEVICE where no device is
 * visible (ORB_E_INVALID otherwise).
 * Host pointers; runs on ORBmatcher_stream(h), holds the map handle's lock, synchronous. */
typedef struct orb_loopfuse {
    int nkf;
    const int32_t* kf;           /* nkf */
    const orb_frame* frame;      /* nkf */
    const double* Scw;           /* nkf x 8: q xyzw, t, s */
    int nloop;
    const int32_t* loop_pts;     /* nloop */
    int32_t cur_kf;
    int nmatched;
    const int32_t* matched;      /* nmatched, or NULL: no step 0 */
    float th;                    /* 4 in the reference */
    float logScaleFactor;
    int n_kf_rows;
    const uint8_t* const* kf_desc; /* n_kf_rows pointers */
    int n;                       /* map-point table rows */
    const float* pos;            /* n x 3 */
    const float* normal;         /* n x 3 */
    const float* max_dist;       /* n */
    const float* min_dist;       /* n */
    uint8_t* desc;               /* n x 32, in/out */
    uint8_t* bad;                /* n, in/out */
    int apply, cap_ops, cap_updated;
    int32_t* nfused;             /* out nkf, in the order of kf[] */
    int32_t* ops;                /* out cap_ops x 6 */
    int32_t* updated;            /* out cap_updated */
    int32_t n_ops, n_updated, n_matched_skipped;   /* out */
} orb_loopfuse;
int LoopClosing_SearchAndFuse(ORBmatcher_h h, Map_h map, orb_loopfuse* F);
/* With Map_enable_timing on: ms4 = projection, match (summed over the passes), descriptor
 * recomputation (summed) (HIP events on the matcher's stream) and the host replay (wall clock) of the
 * last LoopClosing_SearchAndFuse; ORB_E_INVALID before the first one. */
int LoopClosing_SearchAndFuse_last_timings(Map_h map, float* ms4);

/* DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) as CSR: strictly ascending
 * node ids, the feature indices of node a at feat[start[a] .. start[a+1]) in insertion order.
 * (Computed by the caller's vocabulary; ORBvoc.txt is not shipped with the reference.) */
typedef struct orb_featvec {
    int n_nodes;
    const uint32_t* node_id;
    const int32_t* start;
    const int32_t* feat;
} orb_featvec;

/* The searches below take host arrays only (ORBmatcher_set_device_pointers(h, 0)).  The
 * device enumerates every window / vocabulary-node candidate with its Hamming distance; the
 * order-dependent selection is replayed on the host, in the reference's order. */

/* int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound,
 *                        const float th, const int ORBdist)          ORBmatcher.cc:1472-1599
 * F: CurrentFrame (grid over keysUn, Tcw = mTcw); cur_mp in/out (mvpMapPoints as indices).
 * n = pKF->GetMapPointMatches().size(); kf_mp[i]: map point index or -1; skip[i] = isBad() ||
 * sAlreadyFound.count(pMP); kf_angle[i] = pKF->mvKeysUn[i].angle.  mp_max_dist / mp_min_dist:
 * MapPoint::mfMaxDistance / mfMinDistance; logScaleFactor = CurrentFrame.mfLogScaleFactor. */
int ORBmatcher_SearchByProjection_KeyFrame(ORBmatcher_h h, const orb_frame* F, int32_t* cur_mp, int n,
                                           const int32_t* kf_mp, const uint8_t* skip,
                                           const float* kf_angle, const orb_mappoints* mps,
                                           const float* mp_max_dist, const float* mp_min_dist,
                                           float logScaleFactor, float th, int ORBdist, int* nmatches);

/* int SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
 *                             vector<int>& vnMatches12, int windowSize)  ORBmatcher.cc:405-520
 * prev_matched: F1.N x 2 (in/out); matches12: F1.N (out). */
int ORBmatcher_SearchForInitialization(ORBmatcher_h h, const orb_frame* F1, const orb_frame* F2,
                                       float* prev_matched, int32_t* matches12, int windowSize,
                                       int* nmatches);

/* int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)  ORBmatcher.cc:159-288
 * kf_mp[i]: pKF->GetMapPointMatches()[i] index or -1, kf_mp_bad[i]: isBad(); kf_angle =
 * pKF->mvKeysUn angles, f_angle = F.mvKeys angles; matches[NF] (out): vpMapPointMatches. */
int ORBmatcher_SearchByBoW_Frame(ORBmatcher_h h, int nKF, const uint8_t* kf_desc, const float* kf_angle,
                                 const int32_t* kf_mp, const uint8_t* kf_mp_bad, const orb_featvec* fvKF,
                                 int NF, const uint8_t* f_desc, const float* f_angle,
                                 const orb_featvec* fvF, int32_t* matches, int* nmatches);

/* int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)  ORBmatcher.cc:522-655
 * matches12[n1] (out): the map point of KF2 matched to feature i of KF1, or -1. */
int ORBmatcher_SearchByBoW_KeyFrames(ORBmatcher_h h, int n1, const uint8_t* desc1, const float* angle1,
                                     const int32_t* mp1, const uint8_t* bad1, const orb_featvec* fv1,
                                     int n2, const uint8_t* desc2, const float* angle2,
                                     const int32_t* mp2, const uint8_t* bad2, const orb_featvec* fv2,
                                     int32_t* matches12, int* nmatches);

/* int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12,
 *                            vector<pair<size_t,size_t>>& vMatchedPairs, const bool bOnlyStereo)
 *                                                                    ORBmatcher.cc:657-823
 * KF1/KF2: keysUn, desc, uRight (mvuRight, NULL = all monocular), Tcw, intrinsics, scaleFactors;
 * has_mp[i] = GetMapPoint(i) != NULL; levelSigma2_2 = pKF2->mvLevelSigma2; F12 3x3 row-major.
 * pairs: cap x 2 (idx1, idx2) in idx1 order; *npairs = count (ORB_E_CAPACITY if > cap). */
int ORBmatcher_SearchForTriangulation(ORBmatcher_h h, const orb_frame* KF1, const uint8_t* has_mp1,
                                      const orb_featvec* fv1, const orb_frame* KF2,
                                      const uint8_t* has_mp2, const orb_featvec* fv2,
                                      const float* levelSigma2_2, const float* F12, int bOnlyStereo,
                                      int32_t* pairs, int cap, int* npairs);

/* ---- LocalMapping / LoopClosing projection searches -------------------------------------
 * Map points are the rows of `pts` (GetWorldPos, GetDescriptor) with their
 * orb_mappoint_geo (mfMaxDistance, mfMinDistance, GetNormal).  KeyFrame::GetFeaturesInArea
 * (KeyFrame.cc:569-608, no level filter) and KeyFrame::IsInImage (strict upper bounds)
 * semantics.  Host pointers only (ORB_E_INVALID in device-pointer mode). */
typedef struct orb_mappoint_geo {
    const float* max_dist;     /* MapPoint::mfMaxDistance (n) */
    const float* min_dist;     /* MapPoint::mfMinDistance (n) */
    const float* normal;       /* GetNormal() (n x 3) */
} orb_mappoint_geo;

/* int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 *                        vector<MapPoint*>& vpMatched, int th)      ORBmatcher.cc:290-403
 * pts = vpPoints; skip[i] = isBad() || spAlreadyFound.count(pMP); matched (KF->N, in/out):
 * vpMatched as row indices of pts (-1 = NULL).  KF: keysUn, desc, grid bounds, intrinsics,
 * scaleFactors (Tcw unused: the pose is Scw, 4x4 row-major similarity). */
int ORBmatcher_SearchByProjection_Sim3(ORBmatcher_h h, const orb_frame* KF, const float* Scw,
                                       const orb_mappoints* pts, const orb_mappoint_geo* geo,
                                       const uint8_t* skip, float logScaleFactor, int th,
                                       int32_t* matched, int* nmatches);
/* int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)   825-975
 * skip[i] = !pMP || isBad() || IsInKeyFrame(pKF).  best[i] (out) = keypoint of pKF the
 * reference fuses point i with (bestIdx, 951-971) or -1; *nfused = the return value.  The
 * caller applies 953-969 (Replace / AddObservation) in point order: the selection never
 * depends on those mutations (no occupancy test in Fuse), so the plan is exact -- for this one
 * call.  Across the calls of one LocalMapping::SearchInNeighbors it is not (Replace recomputes the
 * survivor's descriptor; skip and Observations() move): LocalMapping_SearchInNeighbors is that
 * sequence as one exact call. */
int ORBmatcher_Fuse(ORBmatcher_h h, const orb_frame* KF, const orb_mappoints* pts,
                    const orb_mappoint_geo* geo, const uint8_t* skip, float logScaleFactor, float th,
                    int32_t* best, int* nfused);
/* int Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
 *          vector<MapPoint*>& vpReplacePoint)                         977-1100
 * skip[i] = isBad() || pKF->GetMapPoints().count(pMP); best / nfused as Fuse (the caller
 * fills vpReplacePoint[i] from pKF->GetMapPoint(best[i]) or adds the observation). */
int ORBmatcher_Fuse_Sim3(ORBmatcher_h h, const orb_frame* KF, const float* Scw, const orb_mappoints* pts,
                         const orb_mappoint_geo* geo, const uint8_t* skip, float logScaleFactor, float th,
                         int32_t* best, int* nfused);
/* int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12,
 *                  const float& s12, const cv::Mat& R12, const cv::Mat& t12, float th)  1102-1326
 * mp1 (KF1->N) / mp2 (KF2->N): GetMapPointMatches() as rows of pts (-1 = NULL); bad[row] =
 * isBad().  matches12 (KF1->N, in/out): -1 = NULL, >= 0 = the KF2 keypoint of the matched
 * point (GetIndexInKeyFrame(pKF2)), -2 = matched to a point not observed in KF2; every new
 * agreement writes the KF2 keypoint (vpMatches12[i1] = vpMapPoints2[idx2]).  R12: 3x3, t12: 3.
 * KF1's intrinsics project into both keyframes, as in the reference. */
int ORBmatcher_SearchBySim3(ORBmatcher_h h, const orb_frame* KF1, const int32_t* mp1, const orb_frame* KF2,
                            const int32_t* mp2, const orb_mappoints* pts, const orb_mappoint_geo* geo,
                            const uint8_t* bad, float s12, const float* R12, const float* t12,
                            float logScaleFactor, float th, int32_t* matches12, int* nfound);

/* ---- LocalMapping: point creation and map-point updates ---------------------------------
 * Host pointers only (ORB_E_INVALID in device-pointer mode).  Both calls run on
 * ORBmatcher_stream(h) and return after their results are on the host; each packs its inputs
 * into one upload and fetches its results in one download.  Arguments are validated before
 * the device is touched; the handle is looked at last, so a malformed call answers
 * ORB_E_INVALID and a well-formed call with h == NULL answers ORB_E_NODEVICE where no device
 * is visible (ORB_E_INVALID otherwise). */

/* void LocalMapping::CreateNewMapPoints()                         LocalMapping.cc:207-452
 * The geometry applied to every pair SearchForTriangulation returns (262-437), for the
 * current keyframe KF1 (mpCurrentKeyFrame) and `count` neighbours, in one kernel launch with
 * one thread per pair.  Per pair: the parallax of the two rays and of the stereo
 * baseline (only the first stereo keypoint's is evaluated: `if / else if`), then
 *   cosParallaxRays < cosParallaxStereo && > 0 && (stereo1 || stereo2 || < 0.9998):
 *       linear triangulation, cv::SVD::compute of the 4x4 float A      status 1
 *   else stereo1 && cosParallaxStereo1 < cosParallaxStereo2: UnprojectStereo(idx1) of KF1  2
 *   else stereo2 && cosParallaxStereo2 < cosParallaxStereo1: UnprojectStereo(idx2) of KF2  3
 *   else                                                                          status 0
 * and the tests in the reference's order: homogeneous w == 0 (-1), z1 <= 0 (-2),
 * z2 <= 0 (-4), reprojection error in KF1 (-3: chi2 5.991 monocular, 7.8
 * stereo) and in KF2 (-5), a zero distance to a camera centre (-6), scale
 * consistency against ratioFactor = 1.5f * scaleFactor (-7).  A pair with status <= 0
 * leaves its x3D / normal / max_dist / min_dist rows untouched.
 * normal / max_dist / min_dist (all three or none): MapPoint::UpdateNormalAndDepth
 * (MapPoint.cc:331-371) of the new point, observations {KF1, KF2}, reference keyframe KF1.
 * The neighbour gates (baseline < mb; baseline / median depth < 0.01) and ComputeF12
 * stay with the caller.  cv::SVD and the float libm calls are restated.
 * KF1 / KF2 fields read: N, keysUn (pt, octave), uRight (NULL = monocular keyframe), Tcw,
 * fx fy cx cy bf b, scaleFactors, nlevels.  depth (mvDepth, N) is required with uRight.
 * ORB_E_INVALID: a null pointer, a negative count, a pair index outside [0, N), an octave
 * outside [0, nlevels). */
typedef struct orb_triangulate {   /* one neighbour keyframe pKF2 */
    const orb_frame* KF2;
    const float* depth2;           /* pKF2->mvDepth (KF2->N) or NULL (monocular) */
    const float* levelSigma2_2;    /* pKF2->mvLevelSigma2 (nlevels) */
    int npairs;
    const int32_t* pairs;          /* npairs x 2 (idx1, idx2): ORBmatcher_SearchForTriangulation's output */
    float* x3D;                    /* out: npairs x 3 */
    int8_t* status;                /* out: npairs */
    float* normal;                 /* out, optional: npairs x 3 */
    float* max_dist;               /* out, optional: npairs */
    float* min_dist;               /* out, optional: npairs */
} orb_triangulate;
int LocalMapping_CreateNewMapPoints_batch(ORBmatcher_h h, const orb_frame* KF1, const float* depth1,
                                          const float* levelSigma2_1, float scaleFactor, int count,
                                          const orb_triangulate* nb);

/* void MapPoint::ComputeDistinctiveDescriptors()                  MapPoint.cc:242-307
 * void MapPoint::UpdateNormalAndDepth()                           MapPoint.cc:331-371
 * for npts map points at once (LocalMapping::ProcessNewKeyFrame, the new points of CreateNewMapPoints,
 * LocalMapping.cc:543-552 after Fuse, and after a loop correction).  Observations are a CSR in
 * mObservations order with bad keyframes already dropped; obs_start[0] == 0 and non-decreasing.
 * Descriptor part (obs_desc != NULL): best[p] = the index, within point p's own observations,
 * of the descriptor with the least median Hamming distance to all of them (the median is
 * sorted(D[i][.])[0.5 * (k - 1)], self distance included; the first index wins a tie), -1 for a
 * point without observations.  Normal part (pos != NULL): normal = sum_i (pos - Ow_i) / |pos -
 * Ow_i| in the given order, divided by the count; max_dist = |pos - ref_Ow| * ref_scale,
 * min_dist = max_dist / ref_scale_top; rows of points without observations are untouched. */
typedef struct orb_pointupdate {
    int npts;
    const int32_t* obs_start;      /* npts + 1 */
    const uint8_t* obs_desc;       /* total x 32: pKF->mDescriptors.row(idx), or NULL */
    int32_t* best;                 /* out: npts */
    const float* pos;              /* npts x 3 (mWorldPos), or NULL */
    const float* obs_Ow;           /* total x 3: pKF->GetCameraCenter() */
    const float* ref_Ow;           /* npts x 3: mpRefKF->GetCameraCenter() */
    const float* ref_scale;        /* npts: mpRefKF->mvScaleFactors[octave of the point's keypoint in mpRefKF] */
    const float* ref_scale_top;    /* npts: mpRefKF->mvScaleFactors[nLevels-1] */
    float* normal;                 /* out: npts x 3 */
    float* max_dist;               /* out: npts */
    float* min_dist;               /* out: npts */
} orb_pointupdate;
int MapPoint_Update_batch(ORBmatcher_h h, const orb_pointupdate* U);

/* Hamming distances for CSR candidate lists (the inner loop of every Search*):
 * query q (descriptor qdesc[q]) against train rows cand[off[q] .. off[q+1]).
 * Writes dist[k] for every candidate k (dist may be NULL: best/second only) and best/second
 * per query (strict '<', earliest candidate wins ties, like the reference loops). */
/* Brute-force matching (SURVEY config 2 (ii): the dense descriptor tile; north star "Hamming
 * brute-force ... over LDS-resident descriptor blocks"): for `count` problems, every query
 * descriptor qdesc[p] (nq[p] x 32) against every train row tdesc[p] (nt[p] x 32); per query the
 * best train index (-1 if none), its distance and the second-best distance (256 if none), by
 * the reference loops' rule (ORBmatcher.cc: DescriptorDistance 1647-1663; best on a strictly
 * smaller distance, so the earliest index wins ties; an equal distance becomes the second).
 * Pointer space per ORBmatcher_set_device_pointers (device mode: enqueued, deferred-chain aware). */
int ORBmatcher_SearchDense_batch(ORBmatcher_h h, int count, const uint8_t* const* qdesc, const int* nq,
                                 const uint8_t* const* tdesc, const int* nt, int32_t* const* best_idx,
                                 int32_t* const* best_dist, int32_t* const* second_dist);
/* Measurement: the last SearchDense_batch's kernel time (ms, HIP events on ORBmatcher_stream,
 * timing on) and its (query, train) pair count. */
int ORBmatcher_last_dense_timing(ORBmatcher_h h, float* ms, long long* pairs);
int ORBmatcher_SearchCandidates(ORBmatcher_h h, const uint8_t* qdesc, int nq,
                                const uint8_t* tdesc, int nt, const int32_t* off,
                                const int32_t* cand, int32_t* dist, int32_t* best_idx,
                                int32_t* best_dist, int32_t* second_dist);

/* ======================================================================
 * RANSAC random stream  (DUtils::Random::RandomInt over glibc rand(),
 * Thirdparty/DBoW2/DUtils/Random.cpp:47-50)
 * The reference draws from the process-global rand() (never seeded on the
 * stereo path => seed 1).  The boundary takes the stream explicitly: an
 * orb_rng is the glibc TYPE_3 additive-feedback state, bit-identical to
 * rand() after srand(seed); the solvers advance it by exactly the draws the
 * reference's loops consume (early returns included).
 * ====================================================================== */
typedef struct orb_rng {
    int32_t tbl[31];
    int32_t f, r;
} orb_rng;
void orb_rng_seed(orb_rng* g, unsigned seed);   /* srand(seed) */
int orb_rng_rand(orb_rng* g);                    /* rand() */

/* ======================================================================
 * PnPsolver  (reference include/PnPsolver.h:59-196, src/PnPsolver.cc)
 * ====================================================================== */
typedef struct PnPsolver_t* PnPsolver_h;

/* PnPsolver(const Frame& F, const vector<MapPoint*>& vpMapPointMatches)  PnPsolver.cc:67-110
 * The adapter packs the N matched, non-bad map points: p3d (N x 3, GetWorldPos),
 * p2d (N x 2, F.mvKeysUn[i].pt), sigma2 (N, F.mvLevelSigma2[octave]),
 * kp_index (N, mvKeyPointIndices) into vpMapPointMatches of size n_matches.
 * SetRansacParameters() defaults are applied as in the reference ctor. */
int PnPsolver_create(int N, const float* p3d, const float* p2d, const float* sigma2,
                     const int32_t* kp_index, int n_matches, float fx, float fy, float cx,
                     float cy, PnPsolver_h* out);
int PnPsolver_destroy(PnPsolver_h h);
/* SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2)  121-157 */
int PnPsolver_set_ransac(PnPsolver_h h, double probability, int minInliers, int maxIterations,
                         int minSet, float epsilon, float th2);
/* cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers) 165-258
 * inliers: n_matches bytes (vbInliers); Tcw: 16 floats (row-major CV_32F 4x4);
 * *has_pose = 0 where the reference returns an empty cv::Mat. */
int PnPsolver_iterate(PnPsolver_h h, int nIterations, orb_rng* rng, int* bNoMore,
                      uint8_t* inliers, int* nInliers, float* Tcw, int* has_pose);
/* `count` independent solvers in one hypothesis launch; solver k draws from rngs[k]
 * (pass the same pointer for all to share one stream in solver order). Per-solver
 * outputs at inliers[k] / Tcw + 16k / bNoMore[k] / nInliers[k] / has_pose[k]. */
int PnPsolver_iterate_batch(int count, PnPsolver_h* hs, int nIterations, orb_rng** rngs,
                            int* bNoMore, uint8_t** inliers, int* nInliers, float* Tcw,
                            int* has_pose);
/* RANSAC bookkeeping (mnIterations, mRansacMaxIts, mRansacMinInliers) */
int PnPsolver_get_state(PnPsolver_h h, int* iterations, int* max_its, int* min_inliers);
/* Measurement (no reference counterpart): HIP-event timing of the calling thread's
 * hypothesis launches.  last_timings: ms2 = {EPnP solve, CheckInliers} of the last timed
 * iterate call, counts2 = {hypotheses, (hypothesis, correspondence) pairs}. */
int PnPsolver_enable_timing(int on);
int PnPsolver_last_timings(float* ms2, long long* counts2);

/* ======================================================================
 * Initializer  (reference include/Initializer.h, src/Initializer.cc): the monocular
 * bootstrap between ORBmatcher_SearchForInitialization and CreateInitialMapMonocular.
 * Host pointers only.  The handle owns its stream and device buffers; every call makes
 * one packed upload, four kernel launches and one download and returns with the
 * results on the host.  Two handles may be used from two threads at once.
 * ====================================================================== */
typedef struct Initializer_t* Initializer_h;

/* Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200)
 * K: 3 x 3 row-major; keys1: n1 x 2, mvKeysUn[i].pt of the reference frame.
 * ORB_E_INVALID: a null pointer, n1 < 0, iterations < 1, sigma <= 0, a non-finite key or K. */
int Initializer_create(const float* K, int n1, const float* keys1, float sigma, int iterations,
                       Initializer_h* out);
int Initializer_destroy(Initializer_h h);

typedef struct orb_init_info {     /* optional diagnostics, all outputs */
    float SH, SF; int use_H;       /* RH = SH/(SH+SF) > 0.40f */
    int best_it_H, best_it_F;      /* iteration whose score won (strict >, earliest wins); -1: none */
    float H21[9], F21[9];
    int n_hyp; int nGood[8]; float parallax[8]; int chosen;   /* 8 (H) or 4 (F) motion hypotheses
                                      (0: the d1/d2 gate failed or no model); chosen = -1 on failure */
    uint8_t* inliersH; uint8_t* inliersF;   /* optional, N matches each (match order), may be NULL */
} orb_init_info;

/* bool Initializer::Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12,
 *                              cv::Mat& R21, cv::Mat& t21, vector<cv::Point3f>& vP3D,
 *                              vector<bool>& vbTriangulated)
 * keys2: n2 x 2; matches12: n1 entries, index into keys2 or -1.  The matches are the pairs
 * (i, matches12[i]) with matches12[i] >= 0 in i order.  rng is advanced by exactly
 * 8 * iterations draws (the caller owns the reference's SeedRandOnce(0): orb_rng_seed(&g, 0)).
 * *ok = the reference's return value.  On *ok == 0 R21, t21, vP3D and vbTriangulated are left
 * untouched; on *ok == 1 vP3D (n1 x 3) and vbTriangulated (n1) hold the chosen hypothesis,
 * zero / false where CheckRT wrote nothing.  info (may be NULL) is always filled.
 * ORB_E_INVALID: a null pointer other than info and its two masks, n2 < 0, a non-finite key, a
 * match index outside [0, n2), or fewer than 8 matches -- the reference would index its
 * 8-point sets out of range there -- or an rng that was never seeded.  ORB_E_CAPACITY from
 * 2^22 reference keys on.  Argument errors are reported before the device is touched and the
 * handle is looked at last (the match checks need its n1): a well-formed call without one
 * answers ORB_E_NODEVICE where no device is visible (ORB_E_INVALID otherwise). */
int Initializer_Initialize(Initializer_h h, int n2, const float* keys2, const int32_t* matches12,
                           orb_rng* rng, float* R21, float* t21, float* vP3D,
                           uint8_t* vbTriangulated, int* ok, orb_init_info* info);
/* Measurement (no reference counterpart): HIP-event times of the handle's next calls.
 * last_timings: ms4 = {hypotheses, select, CheckRT, finish} of the last timed call. */
int Initializer_enable_timing(Initializer_h h, int on);
int Initializer_last_timings(Initializer_h h, float* ms4);

/* ======================================================================
 * Sim3Solver  (reference include/Sim3Solver.h:39-137, src/Sim3Solver.cc)
 * ====================================================================== */
typedef struct Sim3Solver_t* Sim3Solver_h;

/* Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale)  Sim3Solver.cc:37-112
 * The adapter packs the N valid pairs in vpMatched12 order: X1c/X2c (N x 3,
 * Rcw*Xw+tcw of each keyframe = mvX3Dc1/2), sigma2_1/2 (N, mvLevelSigma2[octave]),
 * idx1 (N, mvnIndices1) into vpMatched12 of size N1; K1/K2 = {fx, fy, cx, cy}.
 * SetRansacParameters() defaults (0.99, 6, 300) are applied as in the reference
 * ctor. N must be >= 3 (the reference's loop-closing caller guarantees >= 20). */
int Sim3Solver_create(int N, const float* X1c, const float* X2c, const float* sigma2_1,
                      const float* sigma2_2, const int32_t* idx1, int N1, const float* K1,
                      const float* K2, int bFixScale, Sim3Solver_h* out);
int Sim3Solver_destroy(Sim3Solver_h h);
/* SetRansacParameters(probability, minInliers, maxIterations)  114-138 */
int Sim3Solver_set_ransac(Sim3Solver_h h, double probability, int minInliers, int maxIterations);
/* cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers)  140-207
 * inliers: N1 bytes; T12: 16 floats (row-major 4x4 sim3 [sR t; 0 1]);
 * *has_pose = 0 where the reference returns an empty cv::Mat. */
int Sim3Solver_iterate(Sim3Solver_h h, int nIterations, orb_rng* rng, int* bNoMore,
                       uint8_t* inliers, int* nInliers, float* T12, int* has_pose);
/* `count` independent solvers in one hypothesis launch (LoopClosing::ComputeSim3
 * runs one per loop candidate); same conventions as PnPsolver_iterate_batch. */
int Sim3Solver_iterate_batch(int count, Sim3Solver_h* hs, int nIterations, orb_rng** rngs,
                             int* bNoMore, uint8_t** inliers, int* nInliers, float* T12,
                             int* has_pose);
/* GetEstimatedRotation / GetEstimatedTranslation / GetEstimatedScale  366-379:
 * R (9, row-major), t (3), s of the best hypothesis so far. */
int Sim3Solver_get_estimate(Sim3Solver_h h, float* R, float* t, float* s);
/* (mnIterations, mRansacMaxIts, mRansacMinInliers) */
int Sim3Solver_get_state(Sim3Solver_h h, int* iterations, int* max_its, int* min_inliers);
/* Measurement, as PnPsolver_enable_timing / PnPsolver_last_timings: {ComputeSim3, CheckInliers}. */
int Sim3Solver_enable_timing(int on);
int Sim3Solver_last_timings(float* ms2, long long* counts2);

/* ======================================================================
 * Local bundle adjustment  (reference Optimizer::LocalBundleAdjustment,
 * src/Optimizer.cc:453-778; include/Optimizer.h:45)
 * The adapter gathers lLocalKeyFrames / lLocalMapPoints / lFixedCameras
 * (Optimizer.cc:456-504) and the observations in the order the reference
 * creates its g2o edges (map points in list order, then each point's
 * observation map order, 572-653), and applies the results (Converter
 * round trip, EraseMapPointMatch / EraseObservation, 711-777).
 * Requirements: unique kf_id / pt_id; at most one edge per (keyframe, point).
 * ====================================================================== */
typedef struct ba_problem {
    int n_kf;
    const int32_t* kf_id;      /* KeyFrame::mnId (g2o vertex id) */
    const float* kf_Tcw;       /* n_kf x 16 row-major CV_32F pose */
    const uint8_t* kf_local;   /* 1 = local keyframe (written back; fixed iff mnId == 0), 0 = fixed camera */
    const float* kf_cam;       /* n_kf x 5: fx fy cx cy mbf */
    int n_pt;
    const int32_t* pt_id;      /* MapPoint::mnId */
    const float* pt_pos;       /* n_pt x 3 GetWorldPos() */
    int n_edge;
    const int32_t* edge_pt;    /* index into the points */
    const int32_t* edge_kf;    /* index into the keyframes */
    const float* edge_obs;     /* n_edge x 3: kpUn.pt.x, kpUn.pt.y, mvuRight (< 0 = monocular edge) */
    const float* edge_inv_sigma2;  /* mvInvLevelSigma2[kpUn.octave] */
} ba_problem;

typedef struct ba_result {
    float* kf_Tcw;             /* n_kf x 16 (local keyframes updated, fixed cameras copied) */
    float* pt_pos;             /* n_pt x 3 */
    uint8_t* edge_erase;       /* n_edge: 1 = (pKFi, pMP) pushed to vToErase */
    int32_t iterations[2];     /* optimize(5) / optimize(10) return values */
    int32_t n_erased;
    int32_t aborted;           /* *pbStopFlag was set before optimising: nothing written back */
} ba_result;

/* static void Optimizer::LocalBundleAdjustment(KeyFrame*, bool* pbStopFlag, Map*)
 * stop may be NULL; it is read between LM iterations and trials like g2o's
 * force-stop flag. */
int Optimizer_LocalBundleAdjustment(const ba_problem* P, const volatile bool* stop, ba_result* R);
/* static void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)
 *                                                          Optimizer.cc:49-237
 * (GlobalBundleAdjustemnt, Optimizer.cc:41-47, passes every keyframe and map point.)
 * Every keyframe is a vertex, fixed iff kf_id == 0 (kf_local is ignored); one
 * optimize(nIterations); Huber deltas sqrt(5.99)/sqrt(7.815) when bRobust; no outlier
 * gating.  R->kf_Tcw: every keyframe; R->pt_pos: points with >= 1 edge updated
 * (vbNotIncludedMP points copied); R->iterations[0] = optimize() iterations. */
int Optimizer_BundleAdjustment(const ba_problem* P, int nIterations, int bRobust, const volatile bool* stop,
                               ba_result* R);

/* ======================================================================
 * Sim3 refinement of a loop candidate  (reference Optimizer::OptimizeSim3,
 * src/Optimizer.cc:1046-1241; include/Optimizer.h:56-57; called from
 * LoopClosing::ComputeSim3, LoopClosing.cc:326)
 * One VertexSim3Expmap (numeric Jacobians of EdgeSim3ProjectXYZ and
 * EdgeInverseSim3ProjectXYZ), fixed point vertices, Huber sqrt(th2),
 * optimize(5), chi2 > th2 gating, optimize(10 | 5) on the inliers.
 * ====================================================================== */
typedef struct sim3opt_problem {
    int N;                       /* vpMatches1.size() (= pKF1->N) */
    const uint8_t* valid;        /* N: vpMatches1[i] && pMP1 && !pMP1->isBad() && !pMP2->isBad() && i2 >= 0 */
    const float* X1c;            /* N x 3: R1w*P3D1w + t1w (CV_32F, as Optimizer.cc:1118) */
    const float* X2c;            /* N x 3: R2w*P3D2w + t2w */
    const float* obs1;           /* N x 2: pKF1->mvKeysUn[i].pt */
    const float* obs2;           /* N x 2: pKF2->mvKeysUn[i2].pt */
    const float* inv_sigma2_1;   /* N: pKF1->mvInvLevelSigma2[kpUn1.octave] */
    const float* inv_sigma2_2;   /* N: pKF2->mvInvLevelSigma2[kpUn2.octave] */
    float K1[4], K2[4];          /* fx fy cx cy of pKF1->mK / pKF2->mK */
    float th2;                   /* chi2 threshold (LoopClosing passes 10) */
    int bFixScale;
} sim3opt_problem;

/* static int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale).
 * S12: g2o::Sim3 as 8 doubles (quaternion x y z w = Eigen coeffs(), t, s), in/out; left
 * unchanged on the reference's early return (fewer than 10 inliers after gating).
 * erased: N bytes out, 1 where the reference sets vpMatches1[i] = NULL.
 * *nIn = the return value.  At most 2048 valid correspondences (ORB_E_CAPACITY). */
int Optimizer_OptimizeSim3(const sim3opt_problem* P, double* S12, uint8_t* erased, int* nIn);
/* `count` candidates in one launch (one workgroup each): S12 count x 8, erased[c] N_c bytes. */
int Optimizer_OptimizeSim3_batch(int count, const sim3opt_problem* P, double* S12, uint8_t* const* erased,
                                 int* nIn);

/* ======================================================================
 * Essential-graph optimisation  (reference Optimizer::OptimizeEssentialGraph,
 * src/Optimizer.cc:781-1044; include/Optimizer.h:52-56; called from
 * LoopClosing::CorrectLoop, LoopClosing.cc:567)
 * One VertexSim3Expmap per keyframe, EdgeSim3 with information I7 and no
 * robust kernel (numeric Jacobians), BlockSolver_7_3 without marginalised
 * vertices, Levenberg with setUserLambdaInit(1e-16), optimize(20).
 * Which edges exist (spanning tree, loop edges, covisibility >= minFeat,
 * LoopConnections, de-duplication) is decided by the caller; the same
 * vertex pair may appear in several edges, which are summed.
 * ====================================================================== */
typedef struct essgraph_problem {
    int nKF;                  /* non-bad keyframes, caller's order (>= 1) */
    const double* Scw;        /* nKF x 8 (q xyzw, t, s): vScw, the initial estimates; q of unit length */
    const double* ScwNonCorrected; /* nKF x 8: NonCorrectedSim3[kf] where present, else the Scw row */
    const uint8_t* fixed;     /* nKF: 1 = pLoopKF */
    int nE;
    const int32_t* edge_i;    /* vertex(0) */
    const int32_t* edge_j;    /* vertex(1) */
    const uint8_t* edge_loop; /* 1: LoopConnections edge (both sides from Scw), 0: normal edge */
    int bFixScale;
    int nMP;                  /* map points to correct (0 allowed) */
    const float* mp_pos;      /* nMP x 3 */
    const int32_t* mp_ref;    /* nMP: vertex index of nIDr, -1 = leave the point */
} essgraph_problem;
typedef struct essgraph_result {
    double* Scw;       /* nKF x 8: CorrectedSiw */
    float* Tcw;        /* nKF x 16: the SetPose argument [R | t/s] */
    float* mp_pos;     /* nMP x 3 */
    double* chi2;      /* trace_cap: chi2 before the first solve, then after each */
    int trace_cap, n_solves, lm_trials;
} essgraph_result;

/* static void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3,
 * CorrectedSim3, LoopConnections, bFixScale).  Measurement of edge (i, j): Sjw * Swi, from Scw
 * on a LoopConnections edge, else from ScwNonCorrected.  nIterations: the reference passes 20;
 * 0 evaluates the initial chi2 and does the write-back from the inputs.  A free vertex without
 * an edge is returned unchanged.  n_solves = LM iterations run, lm_trials = factorisations.
 * ORB_E_INVALID (before any device work): null pointers, indices out of range, edge_i ==
 * edge_j, non-finite entries, s <= 0, nIterations < 0.  ORB_E_CAPACITY beyond 458752 edges. */
int Optimizer_OptimizeEssentialGraph(const essgraph_problem* P, int nIterations, essgraph_result* R);

/* ======================================================================
 * Motion-only pose optimisation  (reference Optimizer::PoseOptimization,
 * src/Optimizer.cc:239-451; include/Optimizer.h:48)
 * One SE3 vertex, one unary edge per keypoint with a map point
 * (EdgeSE3ProjectXYZOnlyPose if mvuRight[i] < 0, else the stereo edge),
 * Huber sqrt(5.991) / sqrt(7.815), 4 rounds of optimize(10) each restarted
 * from mTcw, chi2 outlier classification after every round, robust kernel
 * dropped after round 3, early exit when fewer than 10 edges.
 * ====================================================================== */
typedef struct pose_problem {
    int N;                     /* keypoints (pFrame->N) */
    const float* Tcw;          /* 16 row-major pFrame->mTcw */
    const uint8_t* has_mp;     /* N: mvpMapPoints[i] != NULL */
    const float* Xw;           /* N x 3: pMP->GetWorldPos() (rows with has_mp) */
    const float* obs;          /* N x 3: mvKeysUn[i].pt.x, .y, mvuRight[i] */
    const float* inv_sigma2;   /* N: mvInvLevelSigma2[mvKeysUn[i].octave] */
    float fx, fy, cx, cy, bf;  /* pFrame->fx ... mbf */
} pose_problem;

/* static int Optimizer::PoseOptimization(Frame* pFrame).
 * Tcw_out: 16 floats (pFrame->SetPose(toCvMat(SE3quat_recov))); unchanged copy of
 * Tcw when fewer than 3 correspondences.  outlier: N bytes, in/out like
 * pFrame->mvbOutlier -- rows with has_mp are written, the others left as they are.
 * *ninliers = the return value (nInitialCorrespondences - nBad).  At most 8192 map
 * points per frame (ORB_E_CAPACITY). */
int Optimizer_PoseOptimization(const pose_problem* P, float* Tcw_out, uint8_t* outlier, int* ninliers);
/* `count` frames in one launch (one workgroup per frame): Tcw_out count x 16,
 * outlier[f] N_f bytes, ninliers[count]. */
int Optimizer_PoseOptimization_batch(int count, const pose_problem* P, float* Tcw_out, uint8_t* const* outlier,
                                     int* ninliers);

/* Device-resident variant: every array of P[f], Tcw_out[f] (16 floats) and outlier[f]
 * are HIP device pointers (e.g. the matcher's device-mode outputs gathered in HBM);
 * the edges are built on the device.  Synchronous; ninliers is host memory.
 * ORB_E_CAPACITY if a frame has more than 8192 map points (its outputs are not written). */
int Optimizer_PoseOptimization_batch_device(int count, const pose_problem* P, float* const* Tcw_out,
                                            uint8_t* const* outlier, int* ninliers);

/* The frame as PoseOptimization(Frame*) reads it (Optimizer.cc:255-347), every array in
 * device memory: mvpMapPoints as indices into a map-point table (mp[i] = -1: NULL),
 * pMP->GetWorldPos() = mp_pos[3*mp[i]..], mvKeysUn, mvuRight (< 0: monocular edge) and
 * the mvInvLevelSigma2 table indexed by kpUn.octave.  The edges are gathered on the
 * device, so no per-frame host or framework-side packing is needed. */
typedef struct pose_frame {
    int N;
    const float* Tcw;            /* 16 row-major pFrame->mTcw */
    const int32_t* mp;           /* N */
    const float* mp_pos;         /* map point rows, 3 floats each */
    const orb_kp* keysUn;        /* N */
    const float* uRight;         /* N */
    const float* invLevelSigma2; /* nlevels */
    int nlevels;
    float fx, fy, cx, cy, bf;
} pose_frame;
/* Measurement: enable >= 0 switches k_pose_opt timing (HIP events around the launch on the calling
 * thread's pose engine) on or off; last_ms (optional) receives the duration of the last timed
 * launch (waits for it).  ORB_E_INVALID when nothing was timed yet.  No reference counterpart. */
int Optimizer_pose_timing(int enable, float* last_ms);

/* Same outputs and capacity rule as Optimizer_PoseOptimization_batch_device. */
int Optimizer_PoseOptimization_frames_device(int count, const pose_frame* F, float* const* Tcw_out,
                                             uint8_t* const* outlier, int* ninliers);
/* The same, queued on the deferred chain of matcher `chain` (ORBmatcher_set_deferred): behind
 * the chain's earlier calls on ORBmatcher_stream(chain); ninliers[f] is written at
 * ORBmatcher_finish(chain), -1 for a frame over the edge capacity. */
int Optimizer_PoseOptimization_frames_device_deferred(ORBmatcher_h chain, int count, const pose_frame* F,
                                                      float* const* Tcw_out, uint8_t* const* outlier,
                                                      int* ninliers);

/* ----------------------------------------------------------------------
 * Keyframe-block sharded BA across GPUs: one process (or
 * thread) per rank, map points partitioned by the block of their reference
 * keyframe, poses replicated.  Per LM trial the ranks all-reduce the partial
 * Schur complement {S, b_s} and the scalars {chi2, scale, stop}; every rank
 * solves the identical reduced system -- or, with the separator-tree partition
 * (Optimizer_partition_points_nd) of a block-sparse system, each rank factors
 * its own subtrees and only the separators' tiles and rows are exchanged.  Pass each rank the SAME keyframes and
 * its own points + all of their edges (edge order preserved); the results are
 * the rank's points / edges and the (identical) poses.
 * ---------------------------------------------------------------------- */
typedef struct orbgpu_comm_t* orbgpu_comm_h;
/* RCCL over xGMI: rank 0 calls orbgpu_comm_unique_id, the caller distributes the
 * 128 bytes (e.g. MPI / torch.distributed), every rank calls init_rccl with the
 * HIP device it runs on already current.  ORB_E_NODEVICE if librccl is absent. */
int orbgpu_comm_unique_id(uint8_t* id128);
int orbgpu_comm_init_rccl(int nranks, int rank, const uint8_t* id128, orbgpu_comm_h* out);
/* `nranks` in-process ranks (one host thread each, one device): out[0..nranks). */
int orbgpu_comm_init_local(int nranks, orbgpu_comm_h* out);
/* One process per rank on one host (e.g. several ranks sharing one GPU, where RCCL cannot place
 * them): every rank calls this with the same fresh POSIX shm name ("/..."), nranks and
 * max_doubles (the largest exchange, in doubles); rank 0 creates the segment, the others attach
 * (bounded wait, ORBGPU_SHM_TIMEOUT s, default 300), and the name is unlinked once all attached.
 * Partials go through host memory and are summed in rank order on every rank (the in-process
 * group's order).  ORB_E_CAPACITY if an exchange exceeds max_doubles. */
int orbgpu_comm_init_shm(const char* name, int nranks, int rank, size_t max_doubles, orbgpu_comm_h* out);
int orbgpu_comm_rank(orbgpu_comm_h h, int* rank, int* size);
int orbgpu_comm_destroy(orbgpu_comm_h h);
/* Keyframe-block partition: pt_rank[p] = rank owning point p.  Reference keyframe
 * of a point = keyframe of its first edge; keyframes in mnId order are cut into
 * nranks contiguous blocks of ~equal edge weight.  Host only (no device needed). */
int Optimizer_partition_points(const ba_problem* P, int nranks, int32_t* pt_rank);
/* Separator-tree partition for the sharded factorisation of a global BA (BundleAdjustment):
 * the nested dissection of the pose graph the engine derives (ordering.hpp), whole subtrees
 * to ranks (nd_assign), each point to the rank of the first subtree pose it observes (a point
 * of separator poses only: round robin).  With it every rank's Schur terms stay inside its own
 * subtrees and the separators, so the ranks factor their subtrees alone and exchange only the
 * separator tiles and rows (Optimizer_BundleAdjustment_sharded checks this and otherwise keeps
 * the replicated factorisation).  Fewer than 24 free poses or one rank: the keyframe-block
 * partition.  kf_owner (optional, n_kf entries): the rank whose subtree holds keyframe k's
 * pose, -1 for a separator pose, -2 for a keyframe that is no free pose; with the
 * keyframe-block fallback, a free pose's owner is its keyframe's block.  Host only. */
int Optimizer_partition_points_nd(const ba_problem* P, int nranks, int32_t* pt_rank, int32_t* kf_owner);
/* The calling thread's last BA run: [sharded factorisation used (0/1), separator tiles and
 * separator rows exchanged per LM trial, Schur-pattern tiles (what the replicated path
 * all-reduces)]. */
int Optimizer_last_sharding(int* info4);
/* The calling thread's last BA run's LM control: info4[0] = steps the device-resident LM queued
 * (k_lm_trial_end decides each trial on the device; a sharded run exchanges between the step's
 * kernels), info4[1] = trials the host loop decided after reading a trial's result back,
 * info4[2] = 1 if the run was sharded over more than one rank, info4[3] = 0. */
int Optimizer_last_lm_path(int* info4);
int Optimizer_LocalBundleAdjustment_sharded(const ba_problem* shard, orbgpu_comm_h comm,
                                            const volatile bool* stop, ba_result* R);
int Optimizer_BundleAdjustment_sharded(const ba_problem* shard, orbgpu_comm_h comm, int nIterations,
                                       int bRobust, const volatile bool* stop, ba_result* R);

/* LM trace of the calling thread's last run (for diagnostics / parity tests):
 * per solve() the initial and final robust chi2, per trial the chi2 and lambda. */
int Optimizer_last_trace(double* solve_ini_chi2, double* solve_chi2, int solve_cap, int* n_solves,
                         double* trial_chi2, double* trial_lambda, int trial_cap, int* n_trials);
/* host milliseconds of the calling thread's last run: [total, structure build] */
int Optimizer_last_timings(double* ms2);

/* Unit entry points of the BA building blocks (parity tests): the dense LDL^T
 * solve of the reduced pose system (variant 0 = register-resident panel kernel,
 * n <= 127; 1 = generic kernel; 2 / 3 = block-sparse tiled, natural / nested-dissection order;
 * 4 = row-owner kernel, n <= 96; 5 / 6 / 7 = column-owner / row-lane / 2-D block-cyclic kernel,
 * n <= 96) and
 * the canonical FP64 sum. */
int orbgpu_unit_ldlt_solve(int n, const double* S, const double* b, double* x, int variant, int* ok);
int orbgpu_unit_csum(const double* v, int n, double* out);
/* tiled LDL^T factorisation only (n x n row-major, upper triangle read): out = d on the
 * diagonal, L in the strict lower triangle, eliminated rows in the strict upper. */
int orbgpu_unit_ldlt_factor(int n, const double* S, double* out);
/* PnPsolver batch work-area layout invariant (host only, no device): for n solvers with
 * N[k] correspondences, K[k] hypotheses and minSet[k], out4 = {device bytes allocated, device
 * end touched, host bytes allocated, host end touched}; ORB_OK iff everything touched fits. */
int orbgpu_unit_pnp_layout(int n, const int* N, const int* K, const int* minSet, long long* out4);
/* Host only (no device): the BA structure of one optimisation level (csrc/ba_struct.cpp,
 * initializeOptimization + buildIndexMapping + BlockSolver::buildStructure) packed into out:
 * [nE nP nL nBlk nPair | poseKf[nP] | landPt[nL] | ePose[nE] | eLand[nE] | lpStart[nL+1] |
 *  lpList | blkI[nBlk] | blkJ[nBlk] | blkStart[nBlk+1] | pairA[nPair] | pairB[nPair]];
 * ORB_E_CAPACITY when cap (int32 entries) is too small, ORB_E_INVALID on a duplicate
 * (pose, landmark) edge. */
int orbgpu_unit_ba_struct(int nkf, int npt, int ne, const int32_t* edge_kf, const int32_t* edge_pt,
                          const uint8_t* edge_level, const uint8_t* kf_fixed, const int32_t* kf_id,
                          const int32_t* pt_id, int level, int32_t* out, long long cap);
/* The same structure from the builders: gpu = 1 the multi-launch device builder (ba_struct_gpu.hip),
 * gpu = 2 the one-workgroup device builder local-BA sizes run (the multi-launch one outside its
 * limits), gpu = 0 the host restatement.  out = [nE nP nL nBlk nPair nPe nLe nLp |
 * aE | ePose | eLand | poseKf | landPt | peStart | peList | leStart | leList | lpStart | lpList |
 * blkI | blkJ | blkStart | pairA | pairB]; *n_out = its length (ORB_E_CAPACITY beyond cap). */
int orbgpu_unit_ba_struct_all(int nkf, int npt, int ne, const int32_t* edge_kf, const int32_t* edge_pt,
                              const uint8_t* edge_level, const uint8_t* kf_fixed, const int32_t* kf_id,
                              const int32_t* pt_id, int level, int gpu, int32_t* out, long long cap,
                              long long* n_out);
/* one wave's canonical 64-tree of v64[0..64) (cross-lane permlane/DPP path) */
int orbgpu_unit_wave_tree(const double* v64, double* out);
/* The BA kernels' shared-denominator division (SharedDiv, ba_math.hpp) against the plain FP64
 * division on n pairs: out[2i] = SharedDiv(b[i]).div(a[i]), out[2i + 1] = a[i] / b[i]. */
int orbgpu_unit_shared_div(const double* a, const double* b, int n, double* out);
/* Test knob: the BA chi2 canonical sum keeps at most m2_max level-2 trees in LDS (default and
 * maximum 1024, i.e. 4.2 M edges) and writes larger sets to its chunk buffer's tail; 0 sends
 * every problem down the tail path.  Process-wide, device-side. */
int orbgpu_unit_set_csum_lds_max(int m2_max);
/* Test knob: computeScale runs in the LM trial's single workgroup for 6 nP + 3 nL <= terms
 * (default and maximum 2048 * 64) and as a chunked two-kernel sum above it; 0 sends every
 * problem down the chunked path.  Process-wide, host-side. */
int orbgpu_unit_set_scale_small_max(int terms);
/* Test knob: BA runs with at least `edges` edges build their structure lists on the device
 * (ba_struct_gpu.hip), smaller ones on the host (default 100000; 0 sends every run to the
 * device builder).  ORBGPU_STRUCT_HOST=1 / 0 in the environment overrides it.  Process-wide. */
int orbgpu_unit_set_struct_gpu_min_edges(int edges);
/* Test knob: an unsharded global BA derives its first pose graph from the caller's edges on the
 * host, beside the device's structure lists; on = 1 also fetches the device's off-diagonal Schur
 * blocks and fails the call (ORB_E_HIP) if the two graphs differ.  Process-wide. */
int orbgpu_unit_set_posegraph_check(int on);
/* The elimination order of the block-sparse pose system (host only, no device): nested
 * dissection of a graph (adjStart[n + 1] / adj: symmetric, sorted lists) with leaves of at
 * most `leaf` nodes; perm[k] = node eliminated k-th; the separator tree's node count and
 * height (0 = a single leaf). */
int orbgpu_unit_nd_order(int n, const int32_t* adjStart, const int32_t* adj, int leaf, int32_t* perm,
                         int32_t* n_nodes, int32_t* height);
/* The Sim3 arithmetic the Sim3 engines share (csrc/sim3_math.hpp) and EdgeSim3::computeError, one
 * thread per item through the engines' own inline functions.  Sim3 rows are 8 doubles (q xyzw, t,
 * s).  op 0: exp, a n x 7 -> out n x 8; 1: log, a n x 8 -> n x 7; 2: a * b -> n x 8; 3: a^-1 ->
 * n x 8; 4: a.map(b), b n x 3 -> n x 3; 5: log(a * b * c^-1) (a = the measurement, b = S_i,
 * c = S_j) -> n x 7.  Unused inputs may be NULL. */
int orbgpu_unit_sim3(int op, int n, const double* a, const double* b, const double* c, double* out);
/* One linearisation and one LM trial of Optimizer_OptimizeEssentialGraph at a given lambda,
 * through the engine's own launches.  Every pointer may be NULL (skipped).  With no edge or no
 * system vertex only nV, sysIdx, meas and the full pass are written and solver = -1. */
typedef struct essgraph_stage {
    int solver;           /* out: 0 dense, 1 tiled (block-sparse, groups of 7 rows) */
    int nV;               /* out: system vertices (free, with an edge); n = 7 nV rows */
    int ok;               /* out: the factorisation met no zero pivot */
    int32_t* sysIdx;      /* nKF: system index, -1 outside the system */
    double* meas;         /* nE x 8 */
    double* err;          /* nE x 7: errors at the linearisation point */
    double* chi2e;        /* nE */
    double* J;            /* nE x 98: [side][row k][column d] */
    double* H;            /* n x n: upper triangle in system order as the solver's storage holds it
                             after the assembly (lambda added), lower triangle 0 */
    double* b;            /* n */
    double* x_solve;      /* n: the solver's x */
    double* x;            /* n: x after the update kernel (scale entries zeroed under bFixScale) */
    double* est_trial;    /* nKF x 8: the trial's estimates */
    double* chi2e_trial;  /* nE */
    double chi2, chi2_trial, scale; /* out: canonical sums (scale without computeScale's 1e-3) */
} essgraph_stage;
int orbgpu_unit_essgraph_stage(const essgraph_problem* P, double lambda, essgraph_stage* out);
/* Test knob: the pose graph's dense single-workgroup solver takes systems of at most `rows` rows
 * (default and maximum 144); 0 sends every system to the block-sparse solver.  Process-wide. */
int orbgpu_unit_set_ess_dense_max(int rows);
/* The SE3 arithmetic PoseOptimization and the BA engines share (csrc/ba_math.hpp: g2o SE3Quat),
 * one thread per item through the kernels' own inline functions.  No reference counterpart.  SE3
 * rows are 7 doubles (q xyzw, t).  op 0: exp, a n x 6 doubles (omega, upsilon) -> out n x 7;
 * 1: a * b -> n x 7; 2: a.map(b), b n x 3 doubles -> n x 3 doubles; 3: Converter::toSE3Quat,
 * a n x 16 FLOATS (row-major Tcw) -> n x 7; 4: the pose write-back, a n x 7 -> out n x 16 FLOATS.
 * b may be NULL where unused. */
int orbgpu_unit_se3(int op, int n, const void* a, const void* b, void* out);
/* One linearisation and one LM trial of Optimizer_PoseOptimization at a given lambda, in one
 * workgroup of `threads` (256 or 512) threads through k_pose_opt's own device functions.  No
 * reference counterpart.  The estimate is toSE3Quat(P->Tcw); edges are the rows with has_mp, in
 * keypoint order; flags holds one byte per edge (bit 0: inactive, bit 1: robust kernel set).
 * Every pointer may be NULL (skipped).  Per-edge outputs of inactive edges are NaN, except
 * keypoint and chi2_class.  At most 8192 edges (ORB_E_CAPACITY). */
typedef struct pose_stage {
    int ne, nA;           /* out: edges, active edges */
    int ok;               /* out: the solve succeeded (0: x is the untouched zero step) */
    int32_t* keypoint;    /* ne: edge -> keypoint index */
    double* T0;           /* 7 */
    double* err;          /* ne x 3 (row 3 of a monocular edge is 0) */
    double* chi2e;        /* ne */
    double* rho;          /* ne: robust chi2 */
    double* J;            /* ne x 18: [row][column], columns (omega, upsilon) */
    double* terms;        /* ne x 28: rho | H upper triangle by rows (21) | b (6) */
    double* sums;         /* 28: the canonical sums of terms over the active edges */
    double* x;            /* 6 */
    double* T_trial;      /* 7: exp(x) * T0 */
    double* chi2e_trial;  /* ne */
    double* rho_trial;    /* ne */
    float* chi2_class;    /* ne: the outlier classification's float chi2 at T_trial */
    float* Tcw_trial;     /* 16: T_trial through the pose write-back */
    double chi2_trial;    /* out: the canonical sum of rho_trial */
    double scale;         /* out: computeScale without its 1e-3 */
} pose_stage;
int orbgpu_unit_pose_stage(const pose_problem* P, const uint8_t* flags, double lambda, int threads, pose_stage* out);
/* Test knob: a KeyFrameDatabase created from now on starts with room for `slots` keyframes and
 * `entries` BowVector entries (defaults 1024 and 1 << 20; both double when full, and the entry
 * pool is compacted when its holes exceed its live entries); 0 restores a default.  Returns 1 on
 * a negative value.  Process-wide, host-side. */
int orbgpu_unit_set_kfdb_initial_capacity(int slots, int entries);
/* Test knobs of the Map handle.  Process-wide, host-side; each returns 1 on a value out of range.
 * initial_capacity: a Map created from now on starts with room for `slots` keyframes, `cells` row
 * slots and map-point ids below `points` (defaults 1024, 1 << 20, 1 << 16; each doubles when
 * full); 0 restores a default.  chunk: Tracking_UpdateLocalMap_batch and
 * KeyFrame_UpdateConnections_batch run at most `frames` queries per launch set (0 = default 64,
 * less where the first-occurrence scratch would pass 256 MiB).  lds_slots: the vote keeps its
 * counters in LDS while the handle has at most `slots` keyframe slots (default and maximum 8192;
 * -1 restores it; 0 sends every vote to counters in device memory). */
int orbgpu_unit_set_map_initial_capacity(int slots, int cells, int points);
int orbgpu_unit_set_map_chunk(int frames);
int orbgpu_unit_set_map_lds_slots(int slots);
/* Instrumented builds only (make prof): read and clear the BA/pose section timers (32 x u64
 * clock64 deltas of workgroup 0); ORB_E_INVALID in normal builds. */
int orbgpu_debug_prof(unsigned long long* out32);
/* Section timers of the matcher's greedy replay kernel (instrumented builds only). */
int orbgpu_debug_prof_match(unsigned long long* out32);
/* Section timers of the FAST cell kernel (instrumented builds only). */
int orbgpu_debug_prof_extract(unsigned long long* out32);
/* Test-only, read-only: what the last successful ORBextractor_extract* call of `h` launched.
 * flags: 1 the pyramid as one launch of tasks (ORBGPU_PYR_FLOW), 2 the top levels chained in one
 * launch (ORBGPU_PYR_CHAIN) from level *chain_from (0: none), 4 FAST split over two streams with
 * both parts non-empty (ORBGPU_FAST_SPLIT), 8 the blur on the side stream (ORBGPU_BLUR_SIDE),
 * 16 the blur right after the pyramid (ORBGPU_BLUR_EARLY), 32 the 32-row resize tile variant
 * (batches of 8 or more).  tile_rows: 2 * nlevels ints, the resize tile height of the 16-row
 * variant per level, then of the 32-row variant (less than 16 / 32 where the source rectangle of
 * a full tile would not fit in LDS).  Every pointer may be NULL.  ORB_E_INVALID before the first
 * successful call. */
int orbgpu_debug_extract_plan(ORBextractor_h h, int* flags, int* chain_from, int* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
