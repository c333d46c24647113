"""cv::remap(src, dst, map1, map2, cv::INTER_LINEAR) restated in numpy: the rectification of
Examples/Stereo/stereo_euroc.cc (BORDER_CONSTANT, value 0, 8-bit, one channel).

TEST INFRASTRUCTURE ONLY -- the checker, never the thing measured.  The specification is OpenCV 3.2
imgwarp.cpp: RemapInvoker's float-map branch, then remapBilinear<FixedPtCast<int, uchar, 15>, ...,
short>.  For a destination pixel with map values mx, my (float32):

  1. sx = cvRound(mx * 32), sy = cvRound(my * 32).  The multiply is a float32 multiply and exact
     (32 is a power of two); cvRound rounds to nearest, ties to even (rintf, and what
     _mm_cvtps_epi32 does in the SIMD path).
  2. ix = sx >> 5, iy = sy >> 5 (arithmetic shift: a floor for negatives); fx = sx & 31,
     fy = sy & 31 on the two's-complement value.  OpenCV saturates ix, iy to short; with sizes up to
     16384 a saturated value is outside the image either way.  A non-finite map value, or one with
     |m * 32| >= 2^30, is treated as far outside, so the pixel is 0: a stated simplification of an
     int conversion that x86 leaves at INT_MIN; the output byte is the same.
  3. The taps S(iy, ix), S(iy, ix+1), S(iy+1, ix), S(iy+1, ix+1): one inside
     [0, src_width) x [0, src_height) reads the source, one outside reads 0.  This one rule covers
     OpenCV's three branches (inlier, fully outside, straddling with BORDER_CONSTANT).
  4. w00 = 32(32-fx)(32-fy), w01 = 32 fx (32-fy), w10 = 32(32-fx) fy, w11 = 32 fx fy: integers that
     sum to 32768.
  5. dst = (S00 w00 + S01 w01 + S10 w10 + S11 w11 + 16384) >> 15; never above 255.

Why the closed form of step 4 is OpenCV's table: initInterTab2D fills BilinearTab_i[fy*32+fx] with
saturate_cast<short>(vy * vx * 32768), vx in {1 - fx/32, fx/32} and vy likewise.  Each product is a
ratio of 5-bit integers, exact in float and exact after scaling.  The only value that does not fit a
short is 32768 at fx = fy = 0; there OpenCV stores 32767 and its sum fix-up adds the missing 1 to
another entry of that 2 x 2 block.  (S00*32767 + S*1 + 16384) >> 15 == S00 for all bytes S00, S (and
a lone (S + 16384) >> 15 is 0), so the closed form with w00 = 32768 gives the same byte in every
case; tests/test_remap_cpu.py checks all 256 x 256 pairs.

cv::remap itself is "parity unpinned" at this OpenCV call site (OpenCV absent, as for cvtColor):
this restatement is pinned on values that follow from the definitions by tests/test_remap_cpu.py."""
import numpy as np

INTER_BITS, INTER_TAB_SIZE, REMAP_COEF_BITS = 5, 32, 15
LIMIT = np.float32(2.0 ** 30)


def weights(fx, fy):
    """Step 4 -> (w00, w01, w10, w11), int64."""
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    return (32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy)


def quantise(map1, map2):
    """Steps 1 and 2 -> (ix, iy, fx, fy, valid): int64 arrays; valid False where a map value is
    non-finite or |m * 32| >= 2^30 (the pixel is 0)."""
    m1, m2 = np.asarray(map1), np.asarray(map2)
    assert m1.dtype == np.float32 and m2.dtype == np.float32 and m1.shape == m2.shape
    with np.errstate(all="ignore"):
        vx, vy = m1 * np.float32(32), m2 * np.float32(32)            # float32 products
        valid = (np.abs(vx) < LIMIT) & (np.abs(vy) < LIMIT)          # NaN, inf: False
    sx = np.rint(np.where(valid, vx, 0)).astype(np.int64)            # to nearest, ties to even
    sy = np.rint(np.where(valid, vy, 0)).astype(np.int64)
    return sx >> 5, sy >> 5, sx & 31, sy & 31, valid


def remap(src, map1, map2):
    """-> dst (uint8, the maps' shape).  src: rows x cols uint8."""
    src = np.asarray(src)
    assert src.ndim == 2 and src.dtype == np.uint8 and src.size > 0
    h, w = src.shape
    ix, iy, fx, fy, valid = quantise(map1, map2)

    def tap(y, x):
        inside = valid & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64), 0)

    w00, w01, w10, w11 = weights(fx, fy)
    acc = tap(iy, ix) * w00 + tap(iy, ix + 1) * w01 + tap(iy + 1, ix) * w10 + tap(iy + 1, ix + 1) * w11
    out = (acc + (1 << (REMAP_COEF_BITS - 1))) >> REMAP_COEF_BITS
    assert out.max(initial=0) <= 255
    return out.astype(np.uint8)
