"""The RGB-D frame input restated in numpy: the cvtColor of Tracking::GrabImage* and
Frame::ComputeStereoFromRGBD with GrabImageRGBD's depth conversion.

TEST INFRASTRUCTURE ONLY -- the checker, never the thing measured.  Both stages are exactly
specified (integer arithmetic; one float32 multiply, one correctly rounded float32 divide and
one subtract), so the GPU tests compare bytes.  cv::cvtColor itself is "parity unpinned"
(OpenCV absent): the constants are OpenCV 3.2's 8-bit path, pinned by tests/test_rgbd_cpu.py."""
import numpy as np

R2Y, G2Y, B2Y, SHIFT = 4899, 9617, 1868, 14   # OpenCV 3.2 color.cpp: yuv_shift = 14


def cvt_gray(img, rgb):
    """cv::cvtColor(img, CV_RGB2GRAY / CV_RGBA2GRAY) for rgb, CV_BGR2GRAY / CV_BGRA2GRAY
    otherwise: (..., 3 | 4) uint8 -> (...) uint8, in int32; a fourth channel is ignored."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] in (3, 4)
    c = img.astype(np.int32)
    first, third = (R2Y, B2Y) if rgb else (B2Y, R2Y)
    g = (c[..., 0] * first + c[..., 1] * G2Y + c[..., 2] * third + (1 << (SHIFT - 1))) >> SHIFT
    return g.astype(np.uint8)


def converts(depth_dtype, factor):
    """GrabImageRGBD's gate: if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F)."""
    diff = np.float32(factor) - np.float32(1.0)
    return abs(float(diff)) > 1e-5 or np.dtype(depth_dtype) != np.float32


def stereo_from_rgbd(keys, keysUn, depth, factor, mbf):
    """-> (mvuRight, mvDepth, keypoints with depth), float32.  depth: rows x cols uint16 / float32
    as loaded.  A keypoint whose truncated (v, u) is outside the image has no depth (the
    library's deliberate difference: the reference would read out of bounds)."""
    depth = np.asarray(depth)
    assert depth.ndim == 2 and depth.dtype in (np.uint16, np.float32)
    rows, cols = depth.shape
    n = len(keys)
    uR = np.full(n, -1, np.float32)
    dep = np.full(n, -1, np.float32)
    if n == 0:
        return uR, dep, 0
    x, y = np.asarray(keys["x"], np.float32), np.asarray(keys["y"], np.float32)
    with np.errstate(invalid="ignore"):
        u, v = np.trunc(x.astype(np.float64)), np.trunc(y.astype(np.float64))   # C++ (int): toward zero
        inside = (u >= 0) & (u < cols) & (v >= 0) & (v < rows)                  # NaN: outside
    ui, vi = u[inside].astype(np.int64), v[inside].astype(np.int64)
    raw = depth[vi, ui]
    with np.errstate(all="ignore"):
        if converts(depth.dtype, factor):
            d = raw.astype(np.float32) * np.float32(factor)   # convertTo(CV_32F, scale): one multiply
        else:
            d = raw.copy()
        ok = d > 0                                            # NaN: no depth; +inf: depth
        idx = np.flatnonzero(inside)[ok]
        dep[idx] = d[ok]
        uR[idx] = np.asarray(keysUn["x"], np.float32)[idx] - np.float32(mbf) / d[ok]
    return uR, dep, int(ok.sum())
