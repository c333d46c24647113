"""Inputs for the RGB-D frame input tests (tests/test_rgbd_cpu.py, tests/test_gpu_rgbd.py):
colour images, depth maps and keypoints, all from seeds."""
import numpy as np

import oracle_lib

TUM_FACTOR = np.float32(1) / np.float32(5000)   # Tracking.cc: mDepthMapFactor = 1.0f / DepthMapFactor (TUM: 5000)
FACTORS = [np.float32(1), np.float32(1) + np.float32(5e-6), TUM_FACTOR, np.float32(2.5)]


def color_image(rng, h, w, ch, kind="random"):
    """random: independent channels (grey equals no channel); primaries: bands of pure R, G, B and
    white (first-byte-R order); ramp: every channel 0..255 across the image, hitting 0 and 255."""
    if kind == "random":
        return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    img = np.zeros((h, w, ch), np.uint8)
    if ch == 4:
        img[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "primaries":
        band = (np.arange(w) * 4) // max(w, 1)
        img[:, band == 0, 0] = 255
        img[:, band == 1, 1] = 255
        img[:, band == 2, 2] = 255
        img[:, band == 3, :3] = 255
        return img
    assert kind == "ramp"
    v = np.round(np.linspace(0, 255, h * w)).astype(np.uint8).reshape(h, w)
    img[..., :3] = v[..., None]
    return img


def spread_gray(rng, gray):
    """Colour images whose channels are random triples "around" a grey image: 3 channels drawn
    independently within +-40 of it (clipped), so no channel equals the grey conversion."""
    g = gray.astype(np.int32)[..., None]
    return np.clip(g + rng.integers(-40, 41, gray.shape + (3,)), 0, 255).astype(np.uint8)


def depth_u16(rng, rows, cols, holes=0.2):
    """About `holes` of the pixels 0 (no measurement), the rest up to 65535, both ends present."""
    d = rng.integers(1, 65536, (rows, cols)).astype(np.uint16)
    d[rng.random((rows, cols)) < holes] = 0
    d.reshape(-1)[:2] = (65535, 0)
    return d


def depth_f32(rng, rows, cols):
    """Metres with zeros, negatives, NaN, +inf and denormals mixed in."""
    d = rng.uniform(0.3, 12.0, (rows, cols)).astype(np.float32)
    k = rng.integers(0, 16, (rows, cols))
    d[k == 0] = 0.0
    d[k == 1] = -d[k == 1]
    d[k == 2] = np.nan
    d[k == 3] = np.inf
    d[k == 4] = np.float32(1e-41)        # denormal
    d[k == 5] = -0.0
    return d


def in_pitch(img, extra_bytes):
    """`img` (2-D) copied into a buffer whose rows are extra_bytes longer (the padding 0xA5 bytes):
    a row stride that need not be a multiple of the element size."""
    rows, cols = img.shape
    pitch = cols * img.itemsize + extra_bytes
    buf = np.full(rows * pitch, 0xA5, np.uint8)
    out = np.ndarray((rows, cols), img.dtype, buf, 0, (pitch, img.itemsize))
    out[...] = img
    return out


# keypoint rows every depth case carries: (x, y) -- inside by truncation, then the out-of-image rule
def special_points(w, h):
    inside = [(0.999, 0.999), (w - 1, h - 1), (w - 0.5, h - 0.5), (-0.5, 3.0)]   # (int)-0.5 == 0
    outside = [(w, 0.0), (0.0, h), (-1.5, 3.0), (np.nan, 2.0), (1e12, 1.0)]
    return inside, outside


def keypoints(rng, n, w, h):
    """-> (mvKeys, mvKeysUn): n records.  Fractional coordinates clipped so that truncation stays
    inside the image (a float32 draw from uniform(0, w) can round up to exactly w); the special
    rows first as far as n allows; keysUn.x differs from keys.x everywhere (an undistortion-like
    shift), so reading the wrong array shows."""
    k = np.zeros(n, oracle_lib.KP_DTYPE)
    x = np.minimum(rng.uniform(0, w, n).astype(np.float32), np.nextafter(np.float32(w), np.float32(0)))
    y = np.minimum(rng.uniform(0, h, n).astype(np.float32), np.nextafter(np.float32(h), np.float32(0)))
    ins, outs = special_points(w, h)
    sp = np.float32(ins + outs)
    m = min(n, len(sp))
    x[:m], y[:m] = sp[:m, 0], sp[:m, 1]
    k["x"], k["y"] = x, y
    k["size"] = np.float32(31)
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.uniform(0, 100, n).astype(np.float32)
    k["octave"] = rng.integers(0, 8, n)
    k["class_id"] = -1
    ku = k.copy()
    ku["x"] = k["x"] + rng.uniform(0.5, 3.0, n).astype(np.float32)
    ku["y"] = k["y"] - rng.uniform(0.5, 3.0, n).astype(np.float32)
    return k, ku
