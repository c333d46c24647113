"""Cases for the cv::remap rectification (tests/remap_ref.py): EuRoC-shaped rectification maps, a
raw stereo pair rendered through the same camera model, and synthetic maps that reach every table
entry, tie, border and special value.

TEST INFRASTRUCTURE ONLY.  euroc_maps() is a float64 numpy statement of what
cv::initUndistortRectifyMap computes (iR = inv(P[:3,:3] @ R), pinhole rays, the Brown-Conrady model,
then astype(float32)); it produces realistic maps and is not claimed to reproduce OpenCV's bits
(OpenCV runs a sum along each row and an LU inverse).  Camera values: Examples/Stereo/EuRoC.yaml
(LEFT / RIGHT .K, .D, .R, .P; 752 x 480)."""
import numpy as np

W, H = 752, 480
_P = [435.2046959714599, 0, 367.4517211914062, 0, 0, 435.2046959714599, 252.2008514404297, 0, 0, 0, 1, 0]
EUROC = {
    "left": dict(
        K=np.array([458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0]).reshape(3, 3),
        D=np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]),
        R=np.array([0.999966347530033, -0.001422739138722922, 0.008079580483432283,
                    0.001365741834644127, 0.9999741760894847, 0.007055629199258132,
                    -0.008089410156878961, -0.007044357138835809, 0.9999424675829176]).reshape(3, 3),
        P=np.array(_P).reshape(3, 4)),
    "right": dict(
        K=np.array([457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0]).reshape(3, 3),
        D=np.array([-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0]),
        R=np.array([0.9999633526194376, -0.003625811871560086, 0.007755443660172947,
                    0.003680398547259526, 0.9999684752771629, -0.007035845251224894,
                    -0.007729688520722713, 0.007064130529506649, 0.999945173484644]).reshape(3, 3),
        P=np.array(_P[:3] + [-47.90639384423901] + _P[4:]).reshape(3, 4)),
}


def distort(x, y, D):
    """Brown-Conrady (k1, k2, p1, p2, k3) on normalised coordinates."""
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    return (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)


def undistort_rectify_maps(K, D, R, P, w, h):
    """cv::initUndistortRectifyMap(K, D, R, P(3x3), (w, h), CV_32F) in float64 -> (map1, map2)
    float32: the raw-image coordinate of every rectified pixel."""
    iR = np.linalg.inv(P[:3, :3] @ R)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    Y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    Wd = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    xd, yd = distort(X / Wd, Y / Wd, D)
    return ((K[0, 0] * xd + K[0, 2]).astype(np.float32), (K[1, 1] * yd + K[1, 2]).astype(np.float32))


def euroc_maps(side):
    c = EUROC[side]
    return undistort_rectify_maps(c["K"], c["D"], c["R"], c["P"], W, H)


def render_raw(scene, side, shift=0.0):
    """The raw (distorted, unrectified) image a EuRoC camera would record of `scene`, a grey image
    in rectified pixel coordinates (shifted `shift` px to the left: a constant disparity).  The
    forward model: every raw pixel is undistorted to its ray (cv::undistortPoints' fixed-point
    iteration, 8 rounds), rotated and projected by R and P, and the scene is sampled there
    bilinearly in float64 (outside: 0)."""
    c = EUROC[side]
    K, D, R, P = c["K"], c["D"], c["R"], c["P"]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x0, y0 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(8):
        xd, yd = distort(x, y, D)
        x, y = x + (x0 - xd), y + (y0 - yd)
    M = P[:3, :3] @ R
    X = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    Y = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    Z = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    px, py = X / Z + shift, Y / Z
    sc = np.asarray(scene, np.float64)
    sh, sw = sc.shape
    jx, jy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    ax, ay = px - jx, py - jy

    def at(yy, xx):
        ok = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        return np.where(ok, sc[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0.0)

    val = ((1 - ay) * ((1 - ax) * at(jy, jx) + ax * at(jy, jx + 1)) +
           ay * ((1 - ax) * at(jy + 1, jx) + ax * at(jy + 1, jx + 1)))
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------- synthetic maps
def table_maps(x0=3, y0=2):
    """32 x 32 destination whose fractions enumerate all 1024 (fx, fy): column = fx, row = fy."""
    f = np.arange(32, dtype=np.float32) / np.float32(32)
    return (np.tile(np.float32(x0) + f, (32, 1)), np.tile((np.float32(y0) + f)[:, None], (1, 32)))


def tie_values(ks=(0, 1, 2, 3, 30, 31, 32, 33, 62, 63, 64, 94, 95, 96)):
    """Every tie k + 0.5 in 1/32 units over a few k, both signs (exact in float32)."""
    k = np.array(ks, np.float64)
    t = (k + 0.5) / 32
    return np.concatenate([t, -t]).astype(np.float32)


def border_values(n):
    """Coordinates along an axis of n source pixels: [-2, 0), ix in {-1, n-1} with zero and
    non-zero fractions, fully outside on both sides, and the special values."""
    v = [-2.0, -1.5, -1.03125, -1.0, -0.96875, -0.5, -0.03125, -0.015625, 0.0, 0.015625, 0.046875, 0.5,
         n - 1.5, n - 1.03125, n - 1.0, n - 0.96875, n - 0.5, n - 0.03125, n - 0.015625, n, n + 0.5, n + 7.0,
         -3.0, -100.0, 40000.0, -40000.0, 1e9, -1e9, 3e9, np.nan, np.inf, -np.inf]
    return np.array(v, np.float32)


def grid_maps(xs, ys):
    """Destination len(ys) x len(xs): pixel (r, c) maps to (xs[c], ys[r])."""
    xs, ys = np.asarray(xs, np.float32), np.asarray(ys, np.float32)
    return (np.tile(xs, (len(ys), 1)), np.tile(ys[:, None], (1, len(xs))))


def random_maps(rng, dw, dh, sw, sh):
    """Arbitrary float32 coordinates from two pixels outside the source to two pixels past it, a
    third of them on the 1/64 grid (ties and exact fractions), a few special values."""
    def axis(n):
        v = rng.uniform(-2.0, n + 1.0, (dh, dw))
        snap = rng.random((dh, dw)) < 1 / 3
        v = np.where(snap, np.rint(v * 64) / 64, v).astype(np.float32)
        sp = rng.random((dh, dw)) < 0.03
        return np.where(sp, rng.choice(np.array([np.nan, np.inf, -np.inf, 1e9, -1e9], np.float32), (dh, dw)), v)
    return axis(sw).astype(np.float32), axis(sh).astype(np.float32)


def source(rng, sh, sw, kind=0):
    """Source bytes: random, or 0 and 255 next to each other (the rounding term decides)."""
    if kind % 2 == 0:
        return rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    return (rng.integers(0, 2, (sh, sw)) * 255).astype(np.uint8)


def in_pitch(a, extra, fill=0):
    """`a` as a view with `extra` more bytes per row (any alignment of the later rows)."""
    a = np.ascontiguousarray(a)
    h, w = a.shape
    row = w * a.itemsize + extra
    buf = np.full(h * row, fill, np.uint8)
    np.lib.stride_tricks.as_strided(buf, (h, w * a.itemsize), (row, 1))[:] = a.view(np.uint8).reshape(h, -1)
    return np.ndarray((h, w), a.dtype, buf, 0, (row, a.itemsize))
