"""CPU: the numpy restatement of the RGB-D frame input (tests/rgbd_ref.py) pinned on values that
follow from the definitions, and the binding / header declarations of the new entry points.

cvtColor: OpenCV 3.2's 8-bit constants (R 4899, G 9617, B 1868, shift 14).  ComputeStereoFromRGBD:
GrabImageRGBD's conversion gate, C++ truncation of the keypoint, d > 0, mvuRight = kpU.x - mbf/d."""
import re

import numpy as np

import oracle_lib
import rgbd_cases as cases
import rgbd_ref as ref
from c_orb_slam_amd import _lib

NEW = ["ORBextractor_cvtColor_batch", "Frame_ComputeStereoFromRGBD", "Frame_ComputeStereoFromRGBD_batch"]


def test_gray_primaries_white_alpha_and_order():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert ref.cvt_gray(px, True).tolist() == [[76, 150, 29, 255, 0]]
    assert ref.cvt_gray(px, False).tolist() == [[29, 150, 76, 255, 0]]
    rng = np.random.default_rng(1)
    img = cases.color_image(rng, 7, 13, 4)
    g = ref.cvt_gray(img, True)
    other = img.copy()
    other[..., 3] = 255 - other[..., 3]
    assert np.array_equal(ref.cvt_gray(other, True), g)                 # alpha ignored
    assert np.array_equal(ref.cvt_gray(img[..., :3], True), g)
    assert np.array_equal(ref.cvt_gray(img[..., [2, 1, 0, 3]], False), g)   # BGR = RGB, ends swapped
    assert not any(np.array_equal(g, img[..., c]) for c in range(3))
    # the integer formula itself, pixel by pixel in Python integers
    r, gg, b = (img[..., c].astype(object) for c in range(3))
    assert np.array_equal(g, ((r * 4899 + gg * 9617 + b * 1868 + 8192) // 16384).astype(np.uint8))
    for kind in ("primaries", "ramp"):
        im = cases.color_image(rng, 4, 64, 3, kind)
        out = ref.cvt_gray(im, True)
        assert out.min() == 0 or kind == "primaries"
        assert out.max() == 255
    assert set(np.unique(ref.cvt_gray(cases.color_image(rng, 2, 64, 3, "primaries"), True))) == {76, 150, 29, 255}
    spread = cases.spread_gray(rng, rng.integers(0, 256, (9, 11), dtype=np.uint8))
    assert spread.shape == (9, 11, 3) and not np.array_equal(spread[..., 0], spread[..., 1])


def _one(x, y, ux, depth, factor, mbf=40.0):
    k = np.zeros(1, oracle_lib.KP_DTYPE)
    k["x"], k["y"] = x, y
    ku = k.copy()
    ku["x"] = ux
    u, d, n = ref.stereo_from_rgbd(k, ku, depth, factor, mbf)
    return u[0], d[0], n


def test_depth_conversion_gate():
    f32 = np.full((4, 4), 2.0, np.float32)
    near1 = np.float32(1) + np.float32(5e-6)
    assert near1 != np.float32(1)
    assert not ref.converts(np.float32, near1) and not ref.converts(np.float32, 1.0)
    assert ref.converts(np.uint16, 1.0) and ref.converts(np.float32, 2.5) and ref.converts(np.float32, cases.TUM_FACTOR)
    assert _one(1.5, 1.5, 9.0, f32, near1)[1] == np.float32(2.0)             # F32, factor ~ 1: untouched
    u16 = np.full((4, 4), 5000, np.uint16)
    assert _one(1.5, 1.5, 9.0, u16, 1.0)[1] == np.float32(5000.0)            # U16, factor 1: converted
    prod = np.float32(5000) * cases.TUM_FACTOR                               # the float product, once
    u, d, n = _one(1.5, 1.5, 9.0, u16, cases.TUM_FACTOR)
    assert d.dtype == np.float32 and d == prod and n == 1
    assert u == np.float32(9.0) - np.float32(40.0) / prod
    assert _one(1.5, 1.5, 9.0, f32, 2.5)[1] == np.float32(5.0)


def test_truncation_and_out_of_image():
    w, h = 6, 5
    depth = (np.arange(h * w, dtype=np.uint16) + 1).reshape(h, w)
    at = lambda x, y: _one(x, y, 100.0, depth, 1.0)[1]
    assert at(0.999, 0.999) == 1                     # (0, 0)
    assert at(w - 1, h - 1) == h * w
    assert at(w - 0.5, h - 0.5) == h * w
    assert at(2.7, 3.2) == depth[3, 2]               # x picks the column, y the row
    assert at(-0.5, 3.0) == depth[3, 0]              # (int)-0.5 == 0
    for x, y in [(w, 0.0), (0.0, h), (-1.5, 3.0), (-1.0, 0.0), (np.nan, 1.0), (1e12, 1.0)]:
        u, d, n = _one(x, y, 100.0, depth, 1.0)
        assert (u, d, n) == (-1, -1, 0), (x, y)
    ins, outs = cases.special_points(w, h)
    k, ku = cases.keypoints(np.random.default_rng(2), 40, w, h)
    small = np.abs(k["x"]) < 1e6                      # 1e12 absorbs the shift, NaN compares unequal
    assert np.all(k["x"][small] != ku["x"][small])
    u, d, n = ref.stereo_from_rgbd(k, ku, depth, 1.0, 40.0)
    assert np.all(d[:len(ins)] > 0) and np.all(d[len(ins):len(ins) + len(outs)] == -1)
    assert np.all(d[len(ins) + len(outs):] > 0)       # the random rows truncate inside the image
    ok = d > 0
    assert np.array_equal(u[ok], ku["x"][ok] - np.float32(40.0) / d[ok]) and n == ok.sum()


def test_nan_inf_zero_negative():
    depth = np.array([[np.nan, np.inf, 0.0, -2.0, -0.0, 1e-41]], np.float32)
    got = [_one(c + 0.5, 0.5, 7.0, depth, 1.0) for c in range(6)]
    assert got[0] == (-1, -1, 0)
    assert got[1] == (np.float32(7.0), np.inf, 1)     # +inf has depth: uRight = kpU.x
    assert got[2] == got[3] == got[4] == (-1, -1, 0)
    assert got[5][1] == np.float32(1e-41) and got[5][0] == -np.inf and got[5][2] == 1   # a denormal is > 0
    # the case generators hold what the tests rely on
    rng = np.random.default_rng(5)
    d = cases.depth_f32(rng, 48, 64)
    assert np.isnan(d).any() and np.isinf(d).any() and (d < 0).any() and (d == 0).any()
    assert ((d > 0) & (d < np.finfo(np.float32).tiny)).any()
    z = cases.depth_u16(rng, 48, 64)
    assert 0.15 < (z == 0).mean() < 0.25 and z.max() == 65535
    p = cases.in_pitch(d, 6)
    assert p.strides == (64 * 4 + 6, 4) and np.array_equal(np.ascontiguousarray(p).view(np.uint8), d.view(np.uint8))


def test_bindings_and_header_declare_the_entries():
    names = _lib.header_functions()
    src = (_lib.PKG / "_lib.py").read_text()
    for n in NEW:
        assert n in names, n
        assert re.search(rf"L\.{n}\.argtypes", src), n
        assert hasattr(_lib.lib(), n), n
    hdr = _lib.HEADER.read_text()
    assert re.search(r"#define ORB_DEPTH_U16 0\b", hdr) and re.search(r"#define ORB_DEPTH_F32 1\b", hdr)
    assert (_lib.ORB_DEPTH_U16, _lib.ORB_DEPTH_F32) == (0, 1)
    fields = [f[0] for f in _lib.orb_rgbd._fields_]
    body = re.search(r"typedef struct orb_rgbd \{(.*?)\} orb_rgbd;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [m for d in body.split(";") for m in re.findall(r"(\w+)\s*(?:,|$)", d.strip())]
    assert declared == fields, (declared, fields)
    # the new entries validate their arguments before they touch a device
    L = _lib.lib()
    assert L.ORBextractor_cvtColor_batch(None, None, 1, 4, 4, 3, 1, 12, 48, 0, None, 4, 16) == _lib.ORB_E_INVALID
    assert L.Frame_ComputeStereoFromRGBD_batch(None, 0, None, None) == _lib.ORB_E_INVALID
    assert L.Frame_ComputeStereoFromRGBD(None, None, None) == _lib.ORB_E_INVALID
